"""coponerf_amd.raster on the MI355X (`pytest -m gpu`): the kernels of csrc/raster.hip against the restatements of
tests/raster_ref.py (pinned on the CPU by tests/test_raster_ref.py), and the module end to end.

Every result is an integer or a bit pattern, so every comparison is EXACT and nothing is left out of one: coverage is integer
arithmetic, and the cases hold no floating-point decision within 1e-9 of a threshold (tests/test_raster_ref.py).  Every output
buffer starts as NaN (floats) or all-ones bytes between guard rows (tests/test_gpu_point_cloud.py: Guarded).  The one
floating-point comparison is photo_check's PSNR: 4 ulp, as tests/test_gpu_splat.py derives it for splat.score.
"""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip, mesh, raster, splat, synthetic as syn
from tests import mesh_ref as mr
from tests import raster_ref as rr
from tests.test_gpu_point_cloud import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                         # a copy: the cases are read-only


def _mesh(case, dev):
    return mesh.Mesh(*(_up(case[k], dev) for k in ("xyz", "rgb", "nvert", "faces", "nface")))


def _host(m):
    """The arrays of a device Mesh as raster_ref takes them: whole capacities, the rows beyond the counts as they are."""
    return {k: getattr(m, k).cpu().numpy() for k in ("xyz", "rgb", "nvert", "faces", "nface")}


def _run(case, dev, cull=0, shade=0, background=(0, 0, 0), outputs=True):
    """The two entry points on guarded buffers -> dict of zbuf (uint64), frames, depth bits (uint32), index and bary, as numpy."""
    m, poses, intr = _mesh(case, dev), _up(case["poses"], dev), _up(case["intrinsics"], dev)
    K, B, H, W = int(poses.shape[0]), int(poses.shape[1]), case["H"], case["W"]
    capv, capf = int(m.xyz.shape[1]), int(m.faces.shape[1])
    n = K * B * H * W
    zbuf, frames = Guarded(n, torch.int64, dev), Guarded(n * 3, torch.uint8, dev)
    depth, index, bary = Guarded(n, torch.float32, dev), Guarded(n, torch.int32, dev), Guarded(n * 3, torch.float32, dev)
    bg = background[0] | background[1] << 8 | background[2] << 16
    _hip.call("cpn_raster_faces", m.xyz.data_ptr(), m.nvert.data_ptr(), m.faces.data_ptr(), m.nface.data_ptr(), poses.data_ptr(),
              intr.data_ptr(), K, B, capv, capf, H, W, cull, rr.NEAR, zbuf.ptr, _hip.stream_handle())
    _hip.call("cpn_raster_resolve", zbuf.ptr, m.xyz.data_ptr(), m.rgb.data_ptr(), m.nvert.data_ptr(), m.faces.data_ptr(),
              poses.data_ptr(), intr.data_ptr(), K, B, capv, capf, H, W, shade, bg, frames.ptr, depth.ptr if outputs else None,
              index.ptr if outputs else None, bary.ptr if outputs else None, _hip.stream_handle())
    shape = (K, B, H, W)
    return dict(zbuf=zbuf.get().view(np.uint64).reshape(shape), frames=frames.get().reshape(shape + (3,)),
                bits=depth.get().view(np.uint32).reshape(shape), index=index.get().reshape(shape),
                bary=bary.get().reshape(shape + (3,)), depth_all=depth.all.cpu().numpy(), index_all=index.all.cpu().numpy(),
                bary_all=bary.all.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("shade", [0, 1])
@pytest.mark.parametrize("cull", [0, 1])
def test_main_against_the_restatement(dev, cull, shade):
    case = rr.main_case()
    bg = (17, 130, 251)
    want = rr.draw(case, cull, shade, background=bg)
    got = _run(case, dev, cull, shade, background=bg)
    rr.same(got, want)
    print("main", cull, shade, "covered pixels", int((want["index"] >= 0).sum()), "of", want["index"].size)
    assert (got["index"][:, 1] == -1).all() and np.isnan(got["bits"][:, 1].view(np.float32)).all()       # pair 1: nface 0
    assert np.isnan(got["bary"][:, 1]).all() and (got["frames"][:, 1] == bg).all() and (got["zbuf"][:, 1] == rr.EMPTY).all()
    assert (got["index"][:, 0] >= 0).any() and (got["index"] < case["hostile"]).all()


@pytest.mark.parametrize("cull", [0, 1])
def test_large_and_small_faces_in_one_wave(dev, cull):
    """Faces of 1, CPN_RASTER_SMALL - 1, CPN_RASTER_SMALL and CPN_RASTER_SMALL + 1 pixels and two that fill the image, in the
    same waves: the one-lane walk and the wave's walk of one launch (tests/test_raster_ref.py checks that the case holds them)."""
    assert rr.SMALL == _hip.CONSTANTS["RASTER_SMALL"]
    case = rr.mixed_case()
    got = _run(case, dev, cull, 0)
    rr.same(got, rr.draw(case, cull, 0))
    if cull == 0:
        assert np.isin(got["index"], rr.MIXED_BIG).any() and (~np.isin(got["index"], rr.MIXED_BIG)).any()


def test_wide_more_tiles_than_workgroups_and_high_face_rows(dev):
    case = rr.wide_case()
    got = _run(case, dev)
    rr.same(got, rr.draw(case))
    assert case["capf"] > 256 * _hip.CONSTANTS["RASTER_TILES"]           # the workgroups of the pair stride: a second tile
    assert case["capf"] > 70000 and (got["index"] > 65535).sum() >= 50


def test_pile_minimum_under_contention_and_the_row_tie(dev):
    case = rr.pile_case()
    got = _run(case, dev)
    rr.same(got, rr.draw(case))
    assert got["index"][0, 0, rr.PILE_A[1], rr.PILE_A[0]] == 0                        # one fp32 depth: the lowest row
    assert got["index"][0, 0, rr.PILE_B[1], rr.PILE_B[0]] == rr.PILE_N + rr.PILE_SPLIT         # the nearer bit pattern first
    assert (got["index"] >= 0).sum() == 2


def test_culling_on_a_closed_sphere(dev):
    """tests/test_raster_ref.py's statements, on the device.  (Reversing every winding of a CLOSED surface cannot draw nothing: the
    far side then winds towards the camera.  It draws none of the faces drawn before; the near side alone, reversed, draws
    nothing.)"""
    case = rr.sphere_case()
    both, front = _run(case, dev, 0), _run(case, dev, 1)
    rr.same(both, rr.draw(case, 0))
    rr.same(front, rr.draw(case, 1))
    covered = both["index"] >= 0
    assert covered.reshape(3, -1).sum(axis=1).min() > 150
    assert np.array_equal(front["index"] >= 0, covered) and np.array_equal(front["zbuf"], both["zbuf"])
    inside_out = _run(rr.reindexed(case, -1), dev, 1)
    rr.same(inside_out, rr.draw(rr.reindexed(case, -1), 1))
    assert np.array_equal(inside_out["index"] >= 0, covered)
    assert not any(np.isin(inside_out["index"][k][covered[k]], front["index"][k][covered[k]]).any() for k in range(3))
    one = rr.near_side(case, 0)
    assert np.array_equal(_run(one, dev, 1)["zbuf"], front["zbuf"][:1])
    assert (_run(rr.reindexed(one, -1), dev, 1)["zbuf"] == rr.EMPTY).all()            # nothing faces the camera


def test_index_order_does_not_matter_on_the_device(dev):
    case = rr.lattice_case()
    base = _run(case, dev)
    rr.same(base, rr.draw(case))
    for how in (1, 2, -1):
        other = _run(rr.reindexed(case, how), dev)
        assert all(np.array_equal(base[what], other[what]) for what in ("zbuf", "index", "bits", "frames"))


def test_null_outputs_leave_their_buffers_alone(dev):
    case = rr.main_case()
    got = _run(case, dev, outputs=False)                                 # .get() has checked the guards of zbuf and frames
    assert np.array_equal(got["frames"], rr.draw(case)["frames"])
    assert np.isnan(got["depth_all"]).all() and (got["index_all"] == -1).all() and np.isnan(got["bary_all"]).all()


def test_the_same_draw_twice_gives_the_same_bytes(dev):
    case = rr.wide_case()                                                # the case with the most contention per pixel
    m, poses, intr = _mesh(case, dev), _up(case["poses"], dev), _up(case["intrinsics"], dev)
    runs = []
    for _ in range(2):
        zbuf = raster.raster_faces(m, poses, intr, case["H"], case["W"])
        out = raster.draw(m, poses, intr, case["H"], case["W"], return_index=True, return_depth=True, return_bary=True)
        runs.append([x.cpu().numpy().tobytes() for x in (zbuf, out["index"], out["frames"], out["depth"], out["bary"])])
    assert runs[0] == runs[1]
    assert runs[0][0] == rr.draw(case)["zbuf"].tobytes()


def test_draw_reads_nothing_on_the_host(dev):
    case = rr.main_case()
    m, poses, intr = _mesh(case, dev), _up(case["poses"], dev), _up(case["intrinsics"], dev)

    def run():
        return raster.draw(m, poses, intr, case["H"], case["W"], cull=True, shade="headlight", background=(1, 2, 3),
                           return_depth=True, return_index=True, return_bary=True)

    run()                                                                # warm up: the library and the kernels are loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = rr.draw(case, 1, 1, background=(1, 2, 3))
    assert set(out) == {"frames", "depth", "index", "bary"}
    assert out["depth"].dtype == torch.float32 and out["index"].dtype == torch.int32 and out["bary"].dtype == torch.float32
    assert np.array_equal(out["frames"].cpu().numpy(), want["frames"]) and np.array_equal(out["index"].cpu().numpy(), want["index"])


def test_bad_arguments_are_status_codes(dev):
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    E_SHAPE, E_ARG = _hip.CONSTANTS["E_SHAPE"], _hip.CONSTANTS["E_ARG"]

    def faces(K=1, B=1, capv=8, capf=8, H=4, W=4, cull=0, near=1e-3, first=p):
        return lib.cpn_raster_faces(first, p, p, p, p, p, K, B, capv, capf, H, W, cull, near, p, s)

    def resolve(K=1, B=1, capv=8, capf=8, H=4, W=4, shade=0, background=0, first=p):
        return lib.cpn_raster_resolve(first, p, p, p, p, p, p, K, B, capv, capf, H, W, shade, background, p, p, p, p, s)

    for bad in (dict(K=0), dict(K=256), dict(H=0), dict(H=16385), dict(W=16385), dict(capf=0), dict(capv=0)):
        assert faces(**bad) == E_SHAPE, bad
        assert b"cpn_raster_faces" in lib.cpn_last_error()
        assert resolve(**bad) == E_SHAPE, bad
        assert b"cpn_raster_resolve" in lib.cpn_last_error()
    for bad in (dict(cull=2), dict(cull=-1), dict(near=0.0), dict(near=float("nan")), dict(first=None)):
        assert faces(**bad) == E_ARG, bad
        assert b"cpn_raster_faces" in lib.cpn_last_error()
    for bad in (dict(shade=2), dict(shade=-1), dict(background=1 << 24), dict(background=-1), dict(first=None)):
        assert resolve(**bad) == E_ARG, bad
        assert b"cpn_raster_resolve" in lib.cpn_last_error()
    torch.cuda.synchronize()
    assert not bool(buf.any())                                           # nothing ran
    m = _mesh(rr.tilted_case(), dev)
    poses, intr = _up(rr.tilted_case()["poses"], dev), _up(rr.tilted_case()["intrinsics"], dev)
    for bad in (dict(H=0, W=4), dict(H=16385, W=4), dict(H=4, W=4, near=0.0)):
        with pytest.raises(ValueError):
            raster.raster_faces(m, poses, intr, **bad)
    zbuf = raster.raster_faces(m, poses, intr, 4, 4)
    for bad in (dict(shade="phong"), dict(background=(0, 0, 256)), dict(background=(0, 0))):
        with pytest.raises(ValueError):
            raster.resolve(zbuf, m, poses, intr, **bad)
    with pytest.raises(ValueError):
        raster.resolve(zbuf.to(torch.int32), m, poses, intr)
    with pytest.raises(ValueError):
        raster.resolve(zbuf, m, poses.expand(2, 1, 4, 4).contiguous(), intr)


# ------------------------------------------------------------------------------------------------------------- end to end
def test_fused_sphere_end_to_end(dev):
    """mesh_ref.chain_case()'s analytic views -> mesh.integrate -> extract on the device -> Mesh.frames in view 0's camera and in
    two orbit cameras, against the restatement applied to that very mesh's arrays."""
    case = mr.chain_case()
    views = {k: _up(case[k], dev) for k in ("depth", "valid", "rgb", "poses")}
    intr = _up(case["intrinsics"], dev)
    surface = mesh.integrate(views, intr, case["S"], dims=case["dims"], bounds=(_up(case["lo"], dev), _up(case["hi"], dev)),
                             trunc_voxels=case["trunc_voxels"]).extract()
    S = case["S"]
    orbit = splat.orbit_poses(1, 3, 3.0, 25.0, pitch_deg=4.0, device=dev)
    poses = torch.cat((views["poses"][:1], orbit[::2]), dim=0).contiguous()          # view 0's camera, and the arc's two ends
    assert torch.equal(poses[0, 0], torch.eye(4, device=dev))
    out = surface.frames(poses, intr, S, S, return_depth=True, return_index=True, return_bary=True)
    assert set(out) == {"frames", "depth", "index", "bary"} and out["frames"].shape == (3, 1, S, S, 3)
    assert set(surface.frames(poses, intr, 20, 28)) == {"frames"}
    host = _host(surface)
    nface = int(host["nface"][0])
    assert 200 < nface <= host["faces"].shape[1] and 200 < int(host["nvert"][0]) <= host["xyz"].shape[1]
    zbuf, band, _ = rr.raster_faces(host, poses.cpu().numpy(), case["intrinsics"], S, S)
    want = rr.resolve(zbuf, host, poses.cpu().numpy(), case["intrinsics"])
    assert not band.any() and not want["band"].any()                     # no decision on a threshold: the comparison is exact
    got = dict(zbuf=raster.raster_faces(surface, poses, intr, S, S).cpu().numpy().view(np.uint64), frames=out["frames"].cpu().numpy(),
               bits=out["depth"].cpu().numpy().view(np.uint32), index=out["index"].cpu().numpy(), bary=out["bary"].cpu().numpy())
    want["zbuf"] = zbuf
    rr.same(got, want)
    share = (got["index"][0] >= 0).mean()
    print("fused sphere: faces", nface, "covered share of view 0", float(share), "of the orbit views",
          [float((got["index"][k] >= 0).mean()) for k in (1, 2)])
    assert share > 0 and (got["index"][1:] >= 0).any()
    light = surface.frames(poses, intr, S, S, shade="headlight")["frames"].cpu().numpy()
    assert np.array_equal(light, rr.resolve(zbuf, host, poses.cpu().numpy(), case["intrinsics"], shade=1)["frames"])
    hit = got["index"][0, 0] >= 0
    assert (light[0, 0][~hit] == 0).all() and len(np.unique(light[0, 0][hit][:, 0])) > 8          # the same faces: not constant
    culled = surface.frames(poses, intr, S, S, cull=True, return_index=True)["index"].cpu().numpy()
    assert np.array_equal(culled[0], got["index"][0])                    # view 0 sees the side the mesh is wound towards


@pytest.fixture(scope="module")
def scene(dev):
    """The synthetic-weight model of the other GPU tests and one pair of 256 x 455 noise photos (tests/test_gpu_splat.py's)."""
    from coponerf_amd import CoPoNeRF
    from coponerf_amd.novel_views import prepare_pair
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    return model, prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)


def test_photo_check_end_to_end(dev, scene):
    """On the synthetic weights the depth is mush and the mesh is empty or nearly so: this only shows that the path runs."""
    model, inp = scene
    coverage, psnr = raster.photo_check(model, inp, dims=(32, 32, 32))
    assert coverage.shape == (2, 1) and psnr.shape == (2, 1) and coverage.dtype == torch.float64 and psnr.dtype == torch.float64
    assert coverage.device.type == "cuda" and psnr.device.type == "cuda"
    c, p = coverage.cpu().numpy(), psnr.cpu().numpy()
    print("photo_check on the synthetic weights: coverage", c.reshape(-1).tolist(), "psnr", p.reshape(-1).tolist())
    assert ((c >= 0) & (c <= 1)).all()
    assert np.array_equal(np.isnan(p), c == 0)
    with pytest.raises(ValueError):
        raster.photo_check(model, inp, t=(0.0, 0.5))
    with pytest.raises(TypeError):
        raster.photo_check(model, inp, radius=1)


PLANE_S, PLANE_DIMS = 64, (40, 40, 24)


def plane_views():
    """tests/test_gpu_splat.py's two overlapping analytic views of the plane z = 4 + 0.3 x + 0.2 y, 64 x 64, with seeded random
    colours and photos and different intrinsics per photo."""
    S, B = PLANE_S, 1
    rng = np.random.default_rng(29)
    intr = np.stack((rr.intrinsics_of(60.0, 58.0, 31.5, 32.2), rr.intrinsics_of(64.0, 61.0, 30.8, 33.1)))[None]      # (B, 2, 4, 4)
    poses = np.stack((np.eye(4, dtype=np.float32), rr.rigid((0.0, 4.0, 0.0), (0.3, 0.05, -0.1))))[:, None]           # (2, B, 4, 4)
    normal, offset = np.array([-0.3, -0.2, 1.0]), 4.0
    v, u = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    K0 = intr[0, 0].astype(np.float64)                                   # render_path renders every view with the query's pinhole
    ray = np.stack(((u - K0[0, 2]) / K0[0, 0], (v - K0[1, 2]) / K0[1, 1], np.ones_like(u)), axis=-1).reshape(-1, 3)
    depth = np.stack([(offset - poses[k, 0, :3, 3].astype(np.float64) @ normal) /
                      ((ray @ poses[k, 0, :3, :3].astype(np.float64).T) @ normal) for k in range(2)]).astype(np.float32)[:, None]
    assert ((depth > 1) & (depth < 9)).all()
    return dict(intr=intr, poses=poses, depth=depth, rgb=rng.uniform(-1, 1, size=(2, B, S * S, 3)).astype(np.float32),
                photos=rng.uniform(-1, 1, size=(B, 2, S, S, 3)).astype(np.float32))


def test_photo_check_wiring_on_a_plane(dev, monkeypatch):
    """The cameras, intrinsics, photos and the order of photo_check's stages, on views that overlap: render_path is replaced by
    the two analytic views of a plane.  The figures must be those of the definition, formed with the restatement on the very mesh
    that integrate and extract make of these views on the device: exact counts, so exact coverage; PSNR to 4 ulp.  The
    post-render stage reads nothing on the host."""
    S, B = PLANE_S, 1
    pv = plane_views()
    views = dict(depth=_up(pv["depth"], dev), valid=torch.ones(2, B, S * S, dtype=torch.uint8, device=dev), poses=_up(pv["poses"], dev),
                 rgb=_up(pv["rgb"], dev), rel_pose=_up(pv["poses"][1], dev))
    inp = {"context": {"rgb": _up(pv["photos"], dev), "intrinsics": _up(pv["intr"], dev)},
           "query": {"intrinsics": _up(pv["intr"][:, :1], dev)}}
    asked = []

    def fake_render_path(model, model_input, t, **kwargs):
        asked.append((tuple(t), kwargs))
        return views

    monkeypatch.setattr(raster, "render_path", fake_render_path)
    raster.photo_check(None, inp, t=(0, 1), dims=PLANE_DIMS)             # warm up: the library and the kernels are loaded
    torch.cuda.synchronize()
    asked.clear()
    torch.cuda.set_sync_debug_mode("error")
    try:
        coverage, psnr = raster.photo_check(None, inp, t=(0, 1), dims=PLANE_DIMS)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    coverage, psnr = coverage.cpu().numpy(), psnr.cpu().numpy()
    assert asked == [((0.0, 1.0), {"window": None, "return_rgb": True, "return_depth": True})]           # rendered once
    surface = mesh.integrate(views, inp["query"]["intrinsics"], S, dims=PLANE_DIMS).extract()
    host = _host(surface)
    assert 500 < int(host["nface"][0]) <= host["faces"].shape[1]
    photo_bytes = np.rint(np.minimum(np.maximum((pv["photos"] + np.float32(1.0)) * np.float32(127.5), 0), 255)).astype(np.uint8)
    for view in (0, 1):
        cam, Kv = pv["poses"][view:view + 1], pv["intr"][:, view]
        zbuf, band, _ = rr.raster_faces(host, cam, Kv, S, S)
        want = rr.resolve(zbuf, host, cam, Kv)
        assert not band.any() and not want["band"].any()
        want_cov, want_psnr = rr.sr.coverage_psnr(rr.sr.score(want["frames"], want["index"], photo_bytes[None, :, view]), S, S)
        print("photo", view, "coverage", float(coverage[view, 0]), "psnr", float(psnr[view, 0]))
        assert want_cov[0, 0] > 0.5 and coverage[view, 0] == want_cov[0, 0]
        assert abs(psnr[view, 0] - want_psnr[0, 0]) <= 4 * 2.0 ** -52 * abs(want_psnr[0, 0])
