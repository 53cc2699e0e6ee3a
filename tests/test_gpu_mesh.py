"""coponerf_amd.mesh on the MI355X (`pytest -m gpu`): the kernels of csrc/mesh.hip element by element against the float64
restatements of tests/mesh_ref.py (pinned on the CPU by tests/test_mesh_ref.py), and reconstruct end to end.

Every output buffer starts as NaN (floats), 0xFF (bytes) or -1 (ints) between guard rows.  The header fixes the float64 operation
sequence and the unit is built without contraction, so the floats are asked for to the same fp32 bits, the integers and bytes
exactly, and EVERY element is compared: tests/test_mesh_ref.py has shown that no decision of any fixture here lies within 1e-9 of
its threshold, so nothing has to be left out.
"""
import warnings

import numpy as np
import pytest
import torch

from coponerf_amd import _hip, synthetic as syn
from tests import mesh_ref as mr
from tests.test_gpu_point_cloud import Guarded
from tests.test_mesh_ref import parse_ply

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                  # a copy: the fixtures are read-only


def _run_integrate(case, dev, pairs=None):
    """cpn_tsdf_integrate on the case (or on the pairs `pairs` of it alone) into guarded buffers -> (tsdf, weight, colour)."""
    sel = slice(None) if pairs is None else pairs
    depth, valid, rgb, poses = (_up(case[k][:, sel], dev) for k in ("depth", "valid", "rgb", "poses"))
    intr, origin, spacing, trunc = (_up(case[k][sel], dev) for k in ("intrinsics", "origin", "spacing", "trunc"))
    K, B, R = depth.shape
    y0, x0, h, w = mr.pr.window_of(case["S"], case["window"])
    Nx, Ny, Nz = case["dims"]
    vox = Nx * Ny * Nz
    tsdf, weight, colour = Guarded(B * vox, torch.float32, dev), Guarded(B * vox, torch.uint8, dev), Guarded(B * vox * 3, torch.float32, dev)
    _hip.call("cpn_tsdf_integrate", depth.data_ptr(), valid.data_ptr(), rgb.data_ptr(), poses.data_ptr(), intr.data_ptr(),
              origin.data_ptr(), spacing.data_ptr(), trunc.data_ptr(), K, B, case["S"], y0, x0, h, w, Nx, Ny, Nz, tsdf.ptr, weight.ptr,
              colour.ptr, _hip.stream_handle())
    return tsdf.get().reshape(B, Nz, Ny, Nx), weight.get().reshape(B, Nz, Ny, Nx), colour.get().reshape(B, Nz, Ny, Nx, 3)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    differ = got.view(np.uint32 if got.dtype == np.float32 else got.dtype) != want.view(np.uint32 if want.dtype == np.float32 else want.dtype)
    print(what, ": elements that differ", int(differ.sum()), "of", differ.size)
    assert not differ.any(), what


# -------------------------------------------------------------------------------------------------------------- integrate
def test_integrate_main_case_bit_for_bit(dev):
    """K = 3, B = 2, S = 16, window (2, 3, 11, 12), dims (9, 7, 5): weight exactly, tsdf and colour to the same fp32 bits, every
    element.  No operation of the device library needed an allowance: +, -, *, / and floor on doubles are correctly rounded."""
    case = mr.main_case()
    ref = mr.integrate_case(case)
    tsdf, weight, colour = _run_integrate(case, dev)
    assert np.array_equal(weight, ref["weight"])
    _same_bits(tsdf, ref["tsdf"], "tsdf")
    _same_bits(colour, ref["colour"], "colour")
    again = _run_integrate(case, dev)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((tsdf, weight, colour), again))          # two runs, the same bytes


@pytest.mark.parametrize("which", [0, 1, 2])
def test_integrate_degenerate_pair(dev, which):
    """trunc = 0, trunc = NaN or a non-positive spacing in pair 1: pair 1 is the empty volume, pair 0 is bit-equal to its result in
    a batch of one."""
    case = mr.degenerate_cases()[which]
    tsdf, weight, colour = _run_integrate(case, dev)
    assert (weight[1] == 0).all() and (tsdf[1] == 1).all() and (colour[1] == 0).all()
    alone = _run_integrate(case, dev, pairs=slice(0, 1))
    for a, b in zip((tsdf, weight, colour), alone):
        assert a[0].tobytes() == b[0].tobytes()
    ref = mr.integrate_case(case)
    assert np.array_equal(weight, ref["weight"]) and weight[0].any()
    _same_bits(tsdf, ref["tsdf"], "tsdf")
    _same_bits(colour, ref["colour"], "colour")


def test_bad_shapes_are_status_codes(dev):
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    E = _hip.CONSTANTS["E_SHAPE"]
    for K, h, n in ((0, 4, 4), (256, 4, 4), (2, 0, 4), (2, 4, 1)):
        assert lib.cpn_tsdf_integrate(p, p, p, p, p, p, p, p, K, 1, 8, 0, 0, h, 4, n, 4, 4, p, p, p, s) == E
        assert b"cpn_tsdf_integrate" in lib.cpn_last_error()
    assert lib.cpn_tsdf_integrate(p, p, p, p, p, p, p, p, 2, 1, 8, 6, 0, 4, 4, 4, 4, 4, p, p, p, s) == E      # the window leaves the grid
    assert lib.cpn_tsdf_integrate(p, p, p, p, p, p, p, p, 2, 1, 8, 0, 0, 4, 4, 2048, 1024, 1024, p, p, p, s) == E  # 2^31 voxels
    for nx, ny, nz in ((1, 4, 4), (4, 4, 1), (1024, 1024, 1024)):
        assert lib.cpn_surface_vertices_scratch(1, nx, ny, nz) == 0 and lib.cpn_surface_faces_scratch(1, nx, ny, nz) == 0
        assert lib.cpn_surface_vertices(p, p, p, p, p, 1, nx, ny, nz, 1, 8, p, p, p, p, p, s) == E
        assert lib.cpn_surface_faces(p, p, 1, nx, ny, nz, 8, p, p, p, s) == E
    assert lib.cpn_surface_vertices_scratch(65536, 2, 2, 2) == 0
    assert lib.cpn_surface_vertices_scratch(2, 17, 13, 9) == 2 * 2 and lib.cpn_surface_faces_scratch(2, 17, 13, 9) == 2 * 6
    torch.cuda.synchronize()
    assert not bool(buf.any())                                   # nothing ran


# ------------------------------------------------------------------------------------------------------------- extraction
def _run_extract(vol, min_weight, capv, capf, dev):
    """The two stages on the volumes `vol` into guarded buffers -> dict of the raw outputs."""
    tsdf, weight, colour, origin, spacing = (_up(vol[k], dev) for k in ("tsdf", "weight", "colour", "origin", "spacing"))
    B, Nz, Ny, Nx = tsdf.shape
    cells = (Nx - 1) * (Ny - 1) * (Nz - 1)
    lib = _hip.lib()
    n_vert, n_face = lib.cpn_surface_vertices_scratch(B, Nx, Ny, Nz), lib.cpn_surface_faces_scratch(B, Nx, Ny, Nz)
    tile = _hip.CONSTANTS["COMPACT_TILE"]
    assert n_vert == B * -(-cells // tile) and n_face == B * -(-3 * Nx * Ny * Nz // tile)
    scratch = torch.empty(max(n_vert, n_face), dtype=torch.int32, device=dev)
    xyz, rgb = Guarded(B * capv * 3, torch.float32, dev), Guarded(B * capv * 3, torch.uint8, dev)
    nvert, cv = Guarded(B, torch.int32, dev), Guarded(B * cells, torch.int32, dev)
    faces, nface = Guarded(B * capf * 3, torch.int32, dev), Guarded(B, torch.int32, dev)
    _hip.call("cpn_surface_vertices", tsdf.data_ptr(), weight.data_ptr(), colour.data_ptr(), origin.data_ptr(), spacing.data_ptr(), B,
              Nx, Ny, Nz, min_weight, capv, scratch.data_ptr(), xyz.ptr, rgb.ptr, nvert.ptr, cv.ptr, _hip.stream_handle())
    _hip.call("cpn_surface_faces", tsdf.data_ptr(), cv.ptr, B, Nx, Ny, Nz, capf, scratch.data_ptr(), faces.ptr, nface.ptr,
              _hip.stream_handle())
    return dict(xyz=xyz.get().reshape(B, capv, 3), rgb=rgb.get().reshape(B, capv, 3), nvert=nvert.get(),
                cell_vertex=cv.get().reshape(B, cells), faces=faces.get().reshape(B, capf, 3), nface=nface.get())


def _check_extract(got, ref, capv, capf):
    """Every element of the six outputs: the counts and cell_vertex exactly, the rows below min(count, capacity) to the same bits,
    the rows beyond untouched."""
    assert np.array_equal(got["nvert"], ref["nvert"]) and np.array_equal(got["nface"], ref["nface"])
    assert np.array_equal(got["cell_vertex"], ref["cell_vertex"])
    for b in range(len(ref["nvert"])):
        n, m = min(int(ref["nvert"][b]), capv), min(int(ref["nface"][b]), capf)
        _same_bits(got["xyz"][b, :n], ref["xyz"][b][:n], f"vert_xyz of pair {b}")
        assert np.array_equal(got["rgb"][b, :n], ref["rgb"][b][:n])
        assert np.array_equal(got["faces"][b, :m], ref["faces"][b][:m])
        assert np.isnan(got["xyz"][b, n:]).all() and (got["rgb"][b, n:] == 255).all() and (got["faces"][b, m:] == -1).all()


@pytest.mark.parametrize("min_weight", [1, 2])
def test_extraction_on_given_volumes(dev, min_weight):
    """dims (17, 13, 9): 1 536 cells and 5 967 lattice edges, past CPN_COMPACT_TILE.  Pair 0 a sphere, pair 1 hostile (random tsdf
    with exact 0, -0, 1 and -1, random weights in {0, 1, 2}, colours with NaN).  Everything exact; vert_xyz to the same bits - no
    operation needed an allowance."""
    case = mr.extract_case()
    ref = mr.extract_of(case, min_weight)
    capv, capf = 1536, 2 * 5967
    got = _run_extract(case, min_weight, capv, capf, dev)
    _check_extract(got, ref, capv, capf)
    again = _run_extract(case, min_weight, capv, capf, dev)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_capacity_below_the_counts(dev):
    """max_vertices and max_faces below the true counts: the counts are still the true ones, the rows beyond the capacity are
    untouched (an odd max_faces: the second triangle of a quad falls outside), and Mesh.numpy raises."""
    from coponerf_amd.mesh import Volume
    case = mr.extract_case()
    ref = mr.extract_of(case, 1)
    capv, capf = 100, 51
    assert (ref["nvert"] > capv).all() and (ref["nface"] > capf).all()
    _check_extract(_run_extract(case, 1, capv, capf, dev), ref, capv, capf)
    vol = Volume(*(_up(case[k], dev) for k in ("tsdf", "weight", "colour", "origin", "spacing")),
                 torch.ones(2, device=dev), case["dims"])
    small = vol.extract(max_vertices=capv, max_faces=capf)
    assert small.xyz.shape == (2, capv, 3) and small.faces.shape == (2, capf, 3)
    assert np.array_equal(small.nvert.cpu().numpy(), ref["nvert"]) and np.array_equal(small.nface.cpu().numpy(), ref["nface"])
    with pytest.raises(RuntimeError, match=f"{int(ref['nvert'][1])} vertices.*max_vertices = {capv}"):
        small.numpy(1)
    assert np.array_equal(small.cloud().count.cpu().numpy(), [capv, capv])
    only_faces = vol.extract(max_faces=capf)                      # room for the vertices, not for the triangles
    with pytest.raises(RuntimeError, match=f"max_faces = {capf}"):
        only_faces.numpy(0)
    full = vol.extract()                                          # the default capacities hold everything
    assert full.xyz.shape == (2, 1536, 3) and full.faces.shape == (2, 3 * 1536, 3)
    for b in range(2):
        xyz, rgb, faces = full.numpy(b)
        assert xyz.tobytes() == ref["xyz"][b].tobytes() and np.array_equal(rgb, ref["rgb"][b]) and np.array_equal(faces, ref["faces"][b])


# ------------------------------------------------------------------------------------------------------------------ chain
def test_chain_sphere_from_four_cameras(dev, tmp_path):
    """Analytic sphere depth from 4 cameras at S = 32 into 24^3 through the Python interface.  The volume equals the restatement's
    bit for bit; the extraction of the GPU's OWN tsdf equals the restatement's extraction of that same array exactly, so a
    last-bit sign flip can never be the question; two runs give the same bytes."""
    from coponerf_amd import mesh
    case = mr.chain_case()
    views = {k: _up(case[k], dev) for k in ("depth", "valid", "rgb", "poses")}
    intr = _up(case["intrinsics"], dev)
    box = (_up(case["lo"], dev), _up(case["hi"], dev))

    def run():
        vol = mesh.integrate(views, intr, case["S"], dims=case["dims"], bounds=box, trunc_voxels=case["trunc_voxels"])
        return vol, vol.extract()

    vol, m = run()
    host = {k: getattr(vol, k).cpu().numpy() for k in ("tsdf", "weight", "colour", "origin", "spacing", "trunc")}
    for k in ("origin", "spacing", "trunc"):
        assert host[k].tobytes() == case[k].tobytes(), k          # the box arithmetic of integrate, in fp32 on the device
    ref = mr.integrate_case(case)
    assert np.array_equal(host["weight"], ref["weight"])
    _same_bits(host["tsdf"], ref["tsdf"], "tsdf")
    _same_bits(host["colour"], ref["colour"], "colour")
    want = mr.extract(host["tsdf"], host["weight"], host["colour"], host["origin"], host["spacing"])
    xyz, rgb, faces = m.numpy(0)
    print("chain: vertices", len(xyz), "triangles", len(faces))
    assert len(xyz) == want["nvert"][0] > 200 and len(faces) == want["nface"][0] > 200
    assert xyz.tobytes() == want["xyz"][0].tobytes() and np.array_equal(rgb, want["rgb"][0]) and np.array_equal(faces, want["faces"][0])
    vol2, m2 = run()
    assert all(torch.equal(getattr(vol, k), getattr(vol2, k)) for k in ("tsdf", "weight", "colour"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip((xyz, rgb, faces), m2.numpy(0)))
    # bounds: the box of the valid points, formed on the device, against numpy on cpn_depth_points' own output
    from coponerf_amd.point_cloud import unproject
    pts = unproject(views["depth"], views["poses"], intr, case["S"]).cpu().numpy().reshape(-1, 3)
    lo, hi = mesh.bounds(views, intr, case["S"])
    ok = ~np.isnan(pts).any(axis=1)
    assert np.array_equal(lo.cpu().numpy()[0], pts[ok].min(axis=0)) and np.array_equal(hi.cpu().numpy()[0], pts[ok].max(axis=0))
    nothing = dict(views, depth=torch.full_like(views["depth"], float("nan")))
    lo, hi = mesh.bounds(nothing, intr, case["S"])
    assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
    empty = mesh.integrate(nothing, intr, case["S"], dims=(8, 8, 8)).extract()       # NaN box: the empty volume, the empty mesh
    assert int(empty.nvert[0]) == 0 and int(empty.nface[0]) == 0
    path = tmp_path / "sphere.ply"
    m.save(path, 0)
    back = parse_ply(path.read_bytes())
    assert back[0].tobytes() == xyz.tobytes() and np.array_equal(back[1], rgb) and np.array_equal(back[2], faces)


# ------------------------------------------------------------------------------------------------------------- end to end
WINDOW = (96, 96, 16, 16)
TS = (0.0, 0.5, 1.0)
DIMS = (16, 16, 16)


def test_reconstruct_end_to_end(dev):
    """mesh.reconstruct on synthetic weights equals integrate + extract on render_path's outputs, and reads nothing on the host.
    The synthetic weights carry no geometry: the mesh may well be EMPTY (the counts are printed), which the equalities survive."""
    from coponerf_amd import CoPoNeRF, mesh, splat
    from coponerf_amd.novel_views import prepare_pair, render_path
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    inp = prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)
    Kq = inp["query"]["intrinsics"]
    views = render_path(model, inp, TS, window=WINDOW, return_rgb=True, return_depth=True)
    vol = mesh.integrate(views, Kq, 256, dims=DIMS, window=WINDOW)
    want = vol.extract()
    assert vol.tsdf.shape == (1, 16, 16, 16) and vol.weight.dtype == torch.uint8 and vol.colour.shape == (1, 16, 16, 16, 3)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                       # nothing is read on the host (the calls above warmed up)
    try:
        got = mesh.reconstruct(model, inp, t=TS, dims=DIMS, window=WINDOW)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            xyz, rgb, faces = got.numpy(0)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert len([c for c in caught if "synchroniz" in str(c.message)]) == 1       # one read
    print("end to end: vertices", len(xyz), "triangles", len(faces), "updated voxels", int((vol.weight > 0).sum()), "of", vol.weight.numel())
    wx, wr, wf = want.numpy(0)
    assert xyz.tobytes() == wx.tobytes() and np.array_equal(rgb, wr) and np.array_equal(faces, wf)
    assert got.xyz.shape == (1, 15 ** 3, 3) and got.faces.shape == (1, 3 * 15 ** 3, 3)
    # against the restatement on the volume's own arrays
    ref = mr.extract(*(getattr(vol, k).cpu().numpy() for k in ("tsdf", "weight", "colour", "origin", "spacing")))
    assert xyz.tobytes() == ref["xyz"][0].tobytes() and np.array_equal(faces, ref["faces"][0])
    # the vertices through the point renderer
    cloud = got.cloud()
    assert int(cloud.count[0]) == len(xyz)
    out = splat.draw(cloud, views["poses"], Kq, 64, 64, return_index=True)
    assert out["frames"].shape == (3, 1, 64, 64, 3) and out["frames"].dtype == torch.uint8
    assert int(out["index"].max()) < max(len(xyz), 1)
