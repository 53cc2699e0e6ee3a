"""coponerf_amd.splat on the MI355X (`pytest -m gpu`): the kernels of csrc/splat.hip against the restatements of
tests/splat_ref.py (pinned on the CPU by tests/test_splat_ref.py), and the module end to end.

Every result is an integer or a bit pattern, so every comparison is EXACT and nothing is left out of one: the cases hold no
point with a decision within 1e-9 of a threshold (tests/test_splat_ref.py).  Every output buffer starts as NaN (floats) or
all-ones bytes between guard rows (tests/test_gpu_point_cloud.py: Guarded).  The one floating-point comparison is
splat.score's PSNR: its argument is formed by the same two correctly rounded float64 operations on both sides, the two log10
(the device library's and numpy's) are each good to 2 ulp and the product with 10 rounds once more: 4 ulp of the value.
"""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip, splat, synthetic as syn
from coponerf_amd.point_cloud import PointCloud
from tests import splat_ref as sr
from tests.test_gpu_point_cloud import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                         # a copy: the cases are read-only


def _cloud(case, dev):
    return PointCloud(_up(case["xyz"], dev), _up(case["rgb"], dev), _up(case["count"], dev))


def _run(case, radius, fill, dev, background=(0, 0, 0), outputs=True):
    """The two entry points on guarded buffers -> dict of zbuf (uint64), frames, depth bits (uint32) and index, as numpy."""
    cloud, poses, intr = _cloud(case, dev), _up(case["poses"], dev), _up(case["intrinsics"], dev)
    K, B, cap, H, W = (case[k] for k in ("K", "B", "cap", "H", "W"))
    n = K * B * H * W
    zbuf, frames = Guarded(n, torch.int64, dev), Guarded(n * 3, torch.uint8, dev)
    depth, index = Guarded(n, torch.float32, dev), Guarded(n, torch.int32, dev)
    bg = background[0] | background[1] << 8 | background[2] << 16
    _hip.call("cpn_splat_points", cloud.xyz.data_ptr(), cloud.count.data_ptr(), poses.data_ptr(), intr.data_ptr(), K, B, cap, H, W,
              radius, sr.NEAR, zbuf.ptr, _hip.stream_handle())
    _hip.call("cpn_splat_resolve", zbuf.ptr, cloud.rgb.data_ptr(), K, B, cap, H, W, fill, bg, frames.ptr,
              depth.ptr if outputs else None, index.ptr if outputs else None, _hip.stream_handle())
    shape = (K, B, H, W)
    return dict(zbuf=zbuf.get().view(np.uint64).reshape(shape), frames=frames.get().reshape(shape + (3,)),
                bits=depth.get().view(np.uint32).reshape(shape), index=index.get().reshape(shape),
                depth_all=depth.all.cpu().numpy(), index_all=index.all.cpu().numpy())


def _same(got, want):
    assert np.array_equal(got["zbuf"], want["zbuf"])
    assert np.array_equal(got["index"], want["index"])
    empty = want["index"] < 0
    assert np.isnan(got["bits"].view(np.float32)[empty]).all()           # NaN where empty,
    assert np.array_equal(got["bits"][~empty], want["bits"][~empty])     # the depth's bits elsewhere
    assert np.array_equal(got["frames"], want["frames"])


# ------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_main_against_the_restatement(dev, radius, fill):
    case = sr.main_case()
    bg = (17, 130, 251)
    want = sr.draw(case, radius, fill, background=bg)
    got = _run(case, radius, fill, dev, background=bg)
    _same(got, want)
    print("main", radius, fill, "covered pixels", int((want["index"] >= 0).sum()), "of", want["index"].size)
    assert (got["index"][:, 1] == -1).all() and np.isnan(got["bits"][:, 1].view(np.float32)).all()       # pair 1: count 0
    assert (got["frames"][:, 1] == bg).all() and (got["zbuf"][:, 1] == sr.EMPTY).all()
    assert (got["index"][:, 0] >= 0).sum() > 0.2 * got["index"][:, 0].size


def test_pile_minimum_under_contention_and_the_index_tie(dev):
    case = sr.pile_case()
    want = sr.draw(case, 0, 0)
    got = _run(case, 0, 0, dev)
    _same(got, want)
    assert got["index"][0, 0, sr.PILE_A[1], sr.PILE_A[0]] == case["nearest"]
    assert got["index"][0, 0, sr.PILE_B[1], sr.PILE_B[0]] == sr.PILE_N


def test_wide_several_workgroups_and_high_indices(dev):
    case = sr.wide_case()
    want = sr.draw(case, 2, 0)
    got = _run(case, 2, 0, dev)
    _same(got, want)
    assert (got["index"] > 65535).sum() > 50


def test_null_outputs_leave_frames_alone(dev):
    case = sr.main_case()
    want = sr.draw(case, 1, 1)
    got = _run(case, 1, 1, dev, outputs=False)                           # .get() has checked the guards of zbuf and frames
    assert np.array_equal(got["frames"], want["frames"])
    assert np.isnan(got["depth_all"]).all() and (got["index_all"] == -1).all()       # not one element of either was written


def test_score_counts_and_figures(dev):
    case = sr.main_case()
    K, B, H, W = (case[k] for k in ("K", "B", "H", "W"))
    drawn = sr.draw(case, 1, 0)
    frames, index = _up(drawn["frames"], dev), _up(drawn["index"], dev)
    rng = np.random.default_rng(5)
    targets = {"self": drawn["frames"], "white": np.full_like(drawn["frames"], 255),
               "random": rng.integers(0, 256, size=drawn["frames"].shape, dtype=np.uint8)}
    n_scratch = _hip.lib().cpn_splat_score_scratch(K, B, H, W)
    assert n_scratch == 2 * K * B * -(-H * W // _hip.CONSTANTS["SPLAT_SCORE_TILE"])
    for name, target in targets.items():
        want = sr.score(drawn["frames"], drawn["index"], target)
        td = _up(target, dev)
        scratch, stats = torch.empty(n_scratch, dtype=torch.int64, device=dev), Guarded(K * B * 2, torch.int64, dev)
        _hip.call("cpn_splat_score", frames.data_ptr(), index.data_ptr(), td.data_ptr(), K, B, H, W, scratch.data_ptr(), stats.ptr,
                  _hip.stream_handle())
        got = stats.get().reshape(K, B, 2)
        print("score", name, got.reshape(-1).tolist())
        assert np.array_equal(got, want)                                 # counts and sums: exact
        assert (want[:, 0, 0] > 0).all() and (want[:, 1] == 0).all() and ((want[:, 0, 1] == 0).all() == (name == "self"))
        cov, psnr = (x.cpu().numpy() for x in splat.score(frames, index, td))
        ref_cov, ref_psnr = sr.coverage_psnr(want, H, W)
        assert cov.dtype == np.float64 and psnr.dtype == np.float64 and cov.shape == (K, B) and psnr.shape == (K, B)
        assert np.array_equal(cov, ref_cov)
        assert np.array_equal(np.isnan(psnr), np.isnan(ref_psnr)) and np.isnan(psnr[:, 1]).all()         # n = 0: NaN
        assert np.array_equal(np.isinf(psnr), np.isinf(ref_psnr)) and (np.isinf(psnr[:, 0]).all() == (name == "self"))
        ok = np.isfinite(ref_psnr)
        assert (np.abs(psnr[ok] - ref_psnr[ok]) <= 4 * 2.0 ** -52 * np.abs(ref_psnr[ok])).all()


def test_score_more_workgroups_than_one_per_image(dev):
    """96 x 96 pixels are three workgroups of CPN_SPLAT_SCORE_TILE pixels per image, the last one not full."""
    rng = np.random.default_rng(6)
    K, B, H, W = 2, 1, 96, 96
    assert H * W > 2 * _hip.CONSTANTS["SPLAT_SCORE_TILE"] and H * W % _hip.CONSTANTS["SPLAT_SCORE_TILE"]
    frames = rng.integers(0, 256, size=(K, B, H, W, 3), dtype=np.uint8)
    target = rng.integers(0, 256, size=(K, B, H, W, 3), dtype=np.uint8)
    index = rng.integers(-1, 3, size=(K, B, H, W)).astype(np.int32)
    got = splat.score_counts(_up(frames, dev), _up(index, dev), _up(target, dev)).cpu().numpy()
    assert np.array_equal(got, sr.score(frames, index, target))


def test_the_same_draw_twice_gives_the_same_bytes(dev):
    case = sr.wide_case()                                                # the case with the most contention per pixel
    cloud, poses, intr = _cloud(case, dev), _up(case["poses"], dev), _up(case["intrinsics"], dev)
    runs = []
    for _ in range(2):
        zbuf = splat.splat_points(cloud, poses, intr, case["H"], case["W"], radius=2)
        out = splat.draw(cloud, poses, intr, case["H"], case["W"], radius=2, fill=1, return_index=True, return_depth=True)
        runs.append([x.cpu().numpy().tobytes() for x in (zbuf, out["index"], out["frames"], out["depth"])])
    assert runs[0] == runs[1]
    assert runs[0][0] == sr.draw(case, 2, 1)["zbuf"].tobytes()


def test_draw_and_score_read_nothing_on_the_host(dev):
    case = sr.main_case()
    cloud, poses, intr = _cloud(case, dev), _up(case["poses"], dev), _up(case["intrinsics"], dev)
    target = _up(sr.draw(case, 1, 1)["frames"], dev)

    def both():
        out = splat.draw(cloud, poses, intr, case["H"], case["W"], radius=1, fill=1, return_depth=True, return_index=True)
        return out, splat.score(out["frames"], out["index"], target)

    both()                                                               # warm up: the library and the kernels are loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, (cov, psnr) = both()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = sr.draw(case, 1, 1)
    assert np.array_equal(out["frames"].cpu().numpy(), want["frames"]) and np.array_equal(out["index"].cpu().numpy(), want["index"])
    assert set(out) == {"frames", "depth", "index"} and out["depth"].dtype == torch.float32 and out["index"].dtype == torch.int32
    assert torch.isinf(psnr[:, 0]).all() and torch.isnan(psnr[:, 1]).all()           # scored against itself; pair 1 is empty


def test_bad_arguments_are_status_codes(dev):
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    E_SHAPE, E_ARG = _hip.CONSTANTS["E_SHAPE"], _hip.CONSTANTS["E_ARG"]
    for K, H in ((0, 4), (256, 4), (2, 0), (2, 2 ** 30)):
        assert lib.cpn_splat_points(p, p, p, p, K, 1, 8, H, 4, 1, 1e-3, p, s) == E_SHAPE
        assert b"cpn_splat_points" in lib.cpn_last_error()
        assert lib.cpn_splat_resolve(p, p, K, 1, 8, H, 4, 0, 0, p, p, p, s) == E_SHAPE
        assert lib.cpn_splat_score(p, p, p, K, 1, H, 4, p, p, s) == E_SHAPE
        assert lib.cpn_splat_score_scratch(K, 1, H, 4) == 0
    assert lib.cpn_splat_points(p, p, p, p, 1, 1, 0, 4, 4, 1, 1e-3, p, s) == E_SHAPE          # cap
    assert lib.cpn_splat_points(p, p, p, p, 1, 1, 8, 4, 4, 9, 1e-3, p, s) == E_ARG            # radius
    assert lib.cpn_splat_points(p, p, p, p, 1, 1, 8, 4, 4, 1, 0.0, p, s) == E_ARG             # near
    assert lib.cpn_splat_resolve(p, p, 1, 1, 8, 4, 4, 5, 0, p, p, p, s) == E_ARG              # fill
    assert lib.cpn_splat_resolve(p, p, 1, 1, 8, 4, 4, 0, 1 << 24, p, p, p, s) == E_ARG        # background
    assert lib.cpn_splat_points(None, p, p, p, 1, 1, 8, 4, 4, 1, 1e-3, p, s) == E_ARG
    torch.cuda.synchronize()
    assert not bool(buf.any())                                           # nothing ran


# ------------------------------------------------------------------------------------------------------------- end to end
WINDOW = (96, 80, 64, 64)


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


def test_reconstruct_orbit_frames_end_to_end(dev, scene):
    """photos -> reconstruct -> orbit_poses -> PointCloud.frames on a 64 x 64 window of the grid, drawn into a 64 x 64 image
    whose principal point is moved by the window's corner.  What the identity camera shows is compared with the restatement
    of this very cloud - whether each point of the synthetic depth falls back on its own pixel is printed, not assumed."""
    from coponerf_amd import point_cloud as pc
    model, inp = scene
    y0, x0, h, w = WINDOW
    Kw = inp["query"]["intrinsics"][:, 0].clone()
    Kw[:, 0, 2] -= x0
    Kw[:, 1, 2] -= y0
    cloud = pc.reconstruct(model, inp, t=(0.0,), min_votes=0, window=WINDOW)
    assert cloud.xyz.shape == (1, h * w, 3)

    poses = splat.orbit_poses(1, 5, 2.0, 30.0, pitch_deg=5.0, device=dev)
    assert poses.shape == (5, 1, 4, 4) and poses.dtype == torch.float32 and poses.device == cloud.xyz.device
    assert torch.equal(splat.orbit_poses(1, 5, 2.0, 30.0, device=dev)[2, 0], torch.eye(4, device=dev))      # no pitch: the middle
    out = cloud.frames(poses, Kw, h, w)
    assert set(out) == {"frames"} and out["frames"].shape == (5, 1, h, w, 3) and out["frames"].dtype == torch.uint8
    out = cloud.frames(poses, Kw, 48, 80, radius=2, fill=2, return_depth=True, return_index=True)
    assert out["frames"].shape == (5, 1, 48, 80, 3) and out["depth"].shape == (5, 1, 48, 80) and out["index"].shape == (5, 1, 48, 80)

    still = splat.orbit_poses(1, 3, 2.0, 0.0, device=dev)                # yaw 0: three identity cameras
    assert torch.equal(still, torch.eye(4, device=dev).expand(3, 1, 4, 4))
    got = cloud.frames(still, Kw, h, w, radius=0, return_depth=True, return_index=True)
    xyz, rgb, count = (x.cpu().numpy() for x in (cloud.xyz, cloud.rgb, cloud.count))
    zbuf, band = sr.splat_points(xyz, count, still.cpu().numpy(), Kw.cpu().numpy(), h, w, 0)
    frames, bits, index = sr.resolve(zbuf, rgb, 0)
    n = int(count[0])
    print("identity camera: points", n, "in the band", int(band.sum()), "pixels that kept a point", int((index[0] >= 0).sum()))
    assert not band.any()                                                # no decision on a threshold: the comparison is exact
    g_index, g_frames = got["index"].cpu().numpy(), got["frames"].cpu().numpy()
    assert np.array_equal(g_index, index) and np.array_equal(g_frames, frames)
    hit = index >= 0
    assert np.array_equal(got["depth"].cpu().numpy().view(np.uint32)[hit], bits[hit])
    assert np.array_equal(g_frames[hit], rgb[0][index[hit]])             # every pixel that kept a point shows that point's colour
    assert np.array_equal(g_index[0], g_index[1]) and np.array_equal(g_index[0], g_index[2])
    assert n > 0 and (index >= 0).any()


def test_cross_view_check_end_to_end(dev, scene):
    model, inp = scene
    coverage, psnr = splat.cross_view_check(model, inp)
    assert coverage.shape == (2, 1) and psnr.shape == (2, 1) and coverage.dtype == torch.float64 and psnr.dtype == torch.float64
    c, p = coverage.cpu().numpy(), psnr.cpu().numpy()
    print("cross_view_check on the synthetic weights: coverage", c.reshape(-1).tolist(), "psnr", p.reshape(-1).tolist())
    assert ((c >= 0) & (c <= 1)).all() and (np.isfinite(p) | np.isnan(p)).all()
    assert np.array_equal(np.isnan(p), c == 0)


def test_cross_view_check_wiring_on_a_plane(dev, monkeypatch):
    """The synthetic weights' pose throws every point out of the other image (coverage 0), so the directions, cameras,
    intrinsics and photos of cross_view_check are checked here on views that overlap: render_path is replaced by the two views
    of a ray-cast plane (64 x 64, the second camera turned 4 degrees and moved 0.3 units: a shift of about 9 of 64 pixels, so
    more than half of either image sees the other), with seeded random colours and photos and different intrinsics per photo.
    The figures must be those of the definition, formed with the restatement: exact counts, so exact coverage, PSNR to 4 ulp."""
    from coponerf_amd import point_cloud as pc
    S, B = 64, 1
    rng = np.random.default_rng(23)
    intr = np.stack((sr.intrinsics_of(60.0, 58.0, 31.5, 32.2), sr.intrinsics_of(64.0, 61.0, 30.8, 33.1)))[None]      # (B, 2, 4, 4)
    poses = np.stack((np.eye(4, dtype=np.float32), sr.rigid((0.0, 4.0, 0.0), (0.3, 0.05, -0.1))))[:, None]           # (2, B, 4, 4)
    normal, offset = np.array([-0.3, -0.2, 1.0]), 4.0                    # the plane z = 4 + 0.3 x + 0.2 y
    v, u = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    K0 = intr[0, 0].astype(np.float64)                                   # render_path renders every view with the query's pinhole
    ray = np.stack(((u - K0[0, 2]) / K0[0, 0], (v - K0[1, 2]) / K0[1, 1], np.ones_like(u)), axis=-1).reshape(-1, 3)
    depth = np.stack([(offset - poses[k, 0, :3, 3].astype(np.float64) @ normal) /
                      ((ray @ poses[k, 0, :3, :3].astype(np.float64).T) @ normal) for k in range(2)]).astype(np.float32)[:, None]
    assert ((depth > 1) & (depth < 9)).all()
    views = dict(depth=_up(depth, dev), valid=torch.ones(2, B, S * S, dtype=torch.uint8, device=dev), poses=_up(poses, dev),
                 rgb=_up(rng.uniform(-1, 1, size=(2, B, S * S, 3)).astype(np.float32), dev), rel_pose=_up(poses[1], dev))
    photos = rng.uniform(-1, 1, size=(B, 2, S, S, 3)).astype(np.float32)
    inp = {"context": {"rgb": _up(photos, dev), "intrinsics": _up(intr, dev)}, "query": {"intrinsics": _up(intr[:, :1], dev)}}
    asked = []

    def fake_render_path(model, model_input, t, **kwargs):
        asked.append((tuple(t), kwargs))
        return views

    monkeypatch.setattr(splat, "render_path", fake_render_path)
    coverage, psnr = (x.cpu().numpy() for x in splat.cross_view_check(None, inp, radius=1, fill=1))
    assert asked == [((0.0, 1.0), {"return_rgb": True, "return_depth": True})]           # rendered once
    photo_bytes = np.rint(np.minimum(np.maximum((photos + np.float32(1.0)) * np.float32(127.5), 0), 255)).astype(np.uint8)
    for src in (0, 1):
        dst = 1 - src
        one = {k: views[k][src:src + 1].contiguous() for k in ("depth", "valid", "rgb", "poses")}
        cloud = pc.from_views(one, inp["query"]["intrinsics"], S, min_votes=0)
        xyz, rgb, count = (x.cpu().numpy() for x in (cloud.xyz, cloud.rgb, cloud.count))
        assert count[0] == S * S
        zbuf, band = sr.splat_points(xyz, count, poses[dst:dst + 1], intr[:, dst], S, S, 1)
        assert not band.any()
        frames, _, index = sr.resolve(zbuf, rgb, 1)
        want_cov, want_psnr = sr.coverage_psnr(sr.score(frames, index, photo_bytes[None, :, dst]), S, S)
        print("direction", src, "coverage", float(coverage[src, 0]), "psnr", float(psnr[src, 0]))
        assert want_cov[0, 0] > 0.5 and coverage[src, 0] == want_cov[0, 0]
        assert abs(psnr[src, 0] - want_psnr[0, 0]) <= 4 * 2.0 ** -52 * abs(want_psnr[0, 0])
