"""tests/mesh_ref.py (the float64 restatement of csrc/mesh.hip that tests/test_gpu_mesh.py compares the kernels with) held to
independent forms on the CPU: a closed formula for the TSDF of a plane, the topology and the volume of an extracted sphere, a
cell worked by hand; the condition on the GPU fixtures (no decision of the rule on its threshold); and the PLY writer."""
import numpy as np
import pytest

from coponerf_amd import _hip
from tests import mesh_ref as mr
from tests import point_cloud_ref as pr


def test_header_declares_the_entry_points():
    for name in ("cpn_tsdf_integrate", "cpn_surface_vertices", "cpn_surface_vertices_scratch", "cpn_surface_faces",
                 "cpn_surface_faces_scratch"):
        assert name in _hip.PROTOTYPES
    assert len(_hip.PROTOTYPES["cpn_tsdf_integrate"][1]) == 22


# ------------------------------------------------------------------------------------------------------------------- TSDF
def test_tsdf_of_a_plane_is_the_clipped_distance():
    """One camera at the identity, a wall at z = d: every pixel's z-depth is d, so a voxel at depth z that falls into the image
    holds min(1, (d - z) / trunc), and nothing where that is below -1."""
    S, d_plane = 32, np.float32(2.37)
    dims = (6, 5, 11)
    intr = np.array([[[40.0, 0, 15.3, 0], [0, 42.0, 16.1, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], dtype=np.float32)
    poses = np.eye(4, dtype=np.float32).reshape(1, 1, 4, 4)
    depth = np.full((1, 1, S * S), d_plane, dtype=np.float32)
    rgb = mr._colours((1, 1, S * S, 3), 3)
    origin = np.array([[-0.2, -0.15, 1.6]], dtype=np.float32)
    spacing = np.array([[0.08, 0.07, 0.13]], dtype=np.float32)
    trunc = np.array([0.31], dtype=np.float32)
    got = mr.integrate(depth, np.ones((1, 1, S * S), np.uint8), rgb, poses, intr, origin, spacing, trunc, S, None, dims)
    z = float(origin[0, 2]) + np.arange(dims[2]).astype(np.float64) * float(spacing[0, 2])
    s = float(d_plane) - z
    seen = s >= -float(trunc[0])
    want = np.where(seen, np.minimum(1.0, s / float(trunc[0])), 1.0).astype(np.float32)
    assert seen.sum() >= 8 and (~seen).sum() >= 2 and (want == 1).sum() >= 3 and (want < 0).sum() >= 2      # every regime occurs
    assert np.array_equal(got["weight"], np.broadcast_to(seen[:, None, None], got["weight"].shape[1:])[None].astype(np.uint8))
    assert got["tsdf"].tobytes() == np.broadcast_to(want[:, None, None], got["tsdf"].shape[1:]).astype(np.float32).tobytes()
    # the colour of a voxel seen by one view is its pixel's: the nearest pixel of the voxel's projection
    iz, iy, ix = 2, 3, 4
    X = origin[0].astype(np.float64) + np.array([ix, iy, iz]) * spacing[0].astype(np.float64)
    c = int(np.floor(40.0 * X[0] / X[2] + float(intr[0, 0, 2]) + 0.5)), int(np.floor(42.0 * X[1] / X[2] + float(intr[0, 1, 2]) + 0.5))
    assert np.array_equal(got["colour"][0, iz, iy, ix], rgb[0, 0, c[1] * S + c[0]])
    assert all(n == 0 for n in got["near"].values())


def test_an_unobserved_pair_is_the_empty_volume():
    case = mr.degenerate_cases()[0]
    got = mr.integrate_case(case)
    assert (got["weight"][1] == 0).all() and (got["tsdf"][1] == 1).all() and (got["colour"][1] == 0).all()
    assert got["weight"][0].any()


# ------------------------------------------------------------------------------------------------------------- extraction
def test_one_cell_by_hand():
    """A 2 x 2 x 2 lattice whose corner 0 alone is inside: the three edges at corner 0 cross, at t = f0 / (f0 - f_other)."""
    f = np.array([-0.25, 0.75, 0.25, 1.0, 0.5, 1.0, 1.0, 1.0], dtype=np.float32).reshape(1, 2, 2, 2)      # [z][y][x]
    colour = np.zeros((1, 2, 2, 2, 3), dtype=np.float32)
    colour[0, 0, 0, 0] = (-1.0, 0.0, 1.0)
    colour[0, 0, 0, 1] = (1.0, 0.0, 1.0)
    origin, spacing = np.array([[1.0, 2.0, 3.0]], np.float32), np.array([[0.5, 2.0, 4.0]], np.float32)
    got = mr.extract(f, np.ones((1, 2, 2, 2), np.uint8), colour, origin, spacing)
    assert got["nvert"][0] == 1 and got["nface"][0] == 0 and got["cell_vertex"].tolist() == [[0]]
    tx, ty, tz = 0.25 / 1.0, 0.25 / 0.5, 0.25 / 0.75
    want = np.array([1.0 + (tx / 3) * 0.5, 2.0 + (ty / 3) * 2.0, 3.0 + (tz / 3) * 4.0])
    assert np.allclose(got["xyz"][0][0], want, rtol=1e-6, atol=0)
    # colours: the x-edge blends (-1, 0, 1) and (1, 0, 1) at t = 1/4, the other two edges blend corner 0 with black
    red = ((0.75 * -1.0 + 0.25 * 1.0) + 0.5 * -1.0 + (2 / 3) * -1.0) / 3
    blue = ((0.75 + 0.25) + 0.5 + 2 / 3) / 3
    assert got["rgb"][0][0].tolist() == [int(np.rint((red + 1) * 127.5)), 128, int(np.rint((blue + 1) * 127.5))]
    # an unobserved corner switches the cell off
    w = np.ones((1, 2, 2, 2), np.uint8)
    w[0, 1, 1, 1] = 0
    assert mr.extract(f, w, colour, origin, spacing)["nvert"][0] == 0
    assert mr.extract(f, w + 1, colour, origin, spacing, min_weight=2)["nvert"][0] == 0
    assert mr.extract(f, w + 1, colour, origin, spacing, min_weight=1)["nvert"][0] == 1


SPHERE_R, SPHERE_C = 0.8, (0.013, -0.021, 0.007)


@pytest.fixture(scope="module")
def sphere():
    dims = (24, 24, 24)
    origin, spacing = np.full((1, 3), -1.15, dtype=np.float32), np.full((1, 3), 0.1, dtype=np.float32)
    sdf = mr.sphere_sdf(dims, origin[0].astype(np.float64), spacing[0].astype(np.float64), SPHERE_C, SPHERE_R).astype(np.float32)[None]
    colour = np.zeros((1, 24, 24, 24, 3), dtype=np.float32)
    weight = np.ones((1, 24, 24, 24), dtype=np.uint8)
    return sdf, weight, colour, origin, spacing, mr.extract(sdf, weight, colour, origin, spacing)


def test_sphere_mesh_is_closed_and_oriented(sphere):
    sdf, weight, colour, origin, spacing, got = sphere
    xyz, faces = got["xyz"][0], got["faces"][0]
    s = float(spacing[0, 0])
    V, F = len(xyz), len(faces)
    assert V == got["nvert"][0] > 500 and F == got["nface"][0] and faces.min() == 0 and faces.max() == V - 1
    edges = mr.edge_counts(faces)
    assert set(edges.values()) == {2}                                    # every undirected edge lies in exactly two triangles
    assert V - len(edges) + F == 2
    vol = mr.signed_volume(xyz, faces)
    lo, hi = 4 / 3 * np.pi * (SPHERE_R - np.sqrt(3) * s) ** 3, 4 / 3 * np.pi * (SPHERE_R + np.sqrt(3) * s) ** 3
    print("sphere: V, E, F", V, len(edges), F, "volume", vol, "in", (lo, hi), "exact", 4 / 3 * np.pi * SPHERE_R ** 3)
    assert 0 < lo < vol < hi
    dist = np.abs(np.linalg.norm(xyz.astype(np.float64) - np.array(SPHERE_C), axis=1) - SPHERE_R)
    assert dist.max() <= np.sqrt(3) * s
    # every directed edge once: the orientation is consistent, not only the sum
    directed = {(t[i], t[(i + 1) % 3]) for t in faces.tolist() for i in range(3)}
    assert len(directed) == 3 * F


def test_flipping_the_sign_flips_the_mesh(sphere):
    sdf, weight, colour, origin, spacing, got = sphere
    flipped = mr.extract(-sdf, weight, colour, origin, spacing)
    assert flipped["xyz"][0].tobytes() == got["xyz"][0].tobytes() and flipped["nface"][0] == got["nface"][0]
    a, b = mr.signed_volume(got["xyz"][0], got["faces"][0]), mr.signed_volume(flipped["xyz"][0], flipped["faces"][0])
    assert a > 0 and b < 0 and abs(a + b) <= 1e-12 * a


def test_cell_vertex_is_a_running_count(sphere):
    cv = sphere[5]["cell_vertex"][0]
    rows = cv[cv >= 0]
    assert np.array_equal(rows, np.arange(len(rows))) and len(rows) == sphere[5]["nvert"][0]


# ---------------------------------------------------------------------------------------------- the GPU tests' fixtures
@pytest.mark.parametrize("name", sorted(mr.gpu_fixtures()))
def test_gpu_fixtures_have_no_decision_on_a_threshold(name):
    got = mr.integrate_case(mr.gpu_fixtures()[name])
    print(name, "near", got["near"], "steps", got["steps"])
    assert got["near"] == dict.fromkeys(mr.DECISIONS, 0)


def test_main_case_reaches_every_step_of_the_rule():
    case = mr.main_case()
    got = mr.integrate_case(case)
    assert all(n > 0 for n in got["steps"].values()), got["steps"]
    d = case["depth"]
    assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d == 0).any() and (d == 10).any()
    assert (case["valid"] == 0).any()
    for b in range(2):
        w = got["weight"][b]
        assert sorted(np.unique(w).tolist()) == [0, 1, 2, 3]
        assert (got["tsdf"][b] < 0).any() and ((got["tsdf"][b] > 0) & (got["tsdf"][b] < 1)).any()
    assert not np.array_equal(got["tsdf"][0], got["tsdf"][1])


def test_extract_fixture_crosses_the_tile_and_is_hostile():
    case = mr.extract_case()
    Nx, Ny, Nz = case["dims"]
    assert (Nx - 1) * (Ny - 1) * (Nz - 1) == 1536 and 3 * Nx * Ny * Nz == 5967 and _hip.CONSTANTS["COMPACT_TILE"] == 1024
    for mw in (1, 2):
        got = mr.extract_of(case, mw)
        print("extract fixture, min_weight", mw, "nvert", got["nvert"], "nface", got["nface"])
    one, two = mr.extract_of(case, 1), mr.extract_of(case, 2)
    assert (one["nvert"] > 100).all() and (one["nface"] > 50).all() and (two["nvert"] < one["nvert"]).all() and (two["nvert"] > 0).all() and \
        (two["nface"] > 0).all()
    t = case["tsdf"][1]
    assert (t == 0).any() and (t == 1).any() and (t == -1).any() and np.signbit(t[t == 0]).any()
    # the hostile volume's mesh is not a manifold: edges in one, two and more triangles all occur
    assert len(set(mr.edge_counts(one["faces"][1]).values())) >= 3
    # the sphere of pair 0 is closed where it is observed everywhere
    whole = mr.extract(case["tsdf"][:1], np.ones_like(case["weight"][:1]), case["colour"][:1], case["origin"][:1], case["spacing"][:1])
    assert set(mr.edge_counts(whole["faces"][0]).values()) == {2} and mr.signed_volume(whole["xyz"][0], whole["faces"][0]) > 0


def test_chain_case_sees_the_sphere():
    case = mr.chain_case()
    got = mr.integrate_case(case)
    assert (~np.isnan(case["depth"])).mean() > 0.1 and np.isnan(case["depth"]).any()
    mesh = mr.extract(got["tsdf"], got["weight"], got["colour"], case["origin"], case["spacing"])
    print("chain: nvert", mesh["nvert"], "nface", mesh["nface"], "weights", np.bincount(got["weight"].reshape(-1)))
    assert mesh["nvert"][0] > 200 and mesh["nface"][0] > 200
    dist = np.abs(np.linalg.norm(mesh["xyz"][0].astype(np.float64) - mr.CHAIN_C, axis=1) - mr.CHAIN_R)
    print("chain: vertices within", float(np.median(dist)), "(median)", float(dist.max()), "(largest) of the sphere")
    assert np.median(dist) < float(case["spacing"].max())


# -------------------------------------------------------------------------------------------------------------------- PLY
def parse_ply(data):
    """(xyz (n, 3) float32, rgb (n, 3) uint8, faces (m, 3) int32) of mesh.ply_bytes' file."""
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == ""
    assert lines[2].startswith("element vertex ") and lines[9].startswith("element face ")
    n, m = int(lines[2].split()[2]), int(lines[9].split()[2])
    assert [tuple(line.split()[1:]) for line in lines[3:9]] == [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"),
                                                                 ("uchar", "green"), ("uchar", "blue")]
    assert lines[10:-1] == ["property list uchar int vertex_indices"]
    assert len(body) == 15 * n + 13 * m
    rows = np.frombuffer(body[:15 * n], dtype=np.uint8).reshape(n, 15)
    tris = np.frombuffer(body[15 * n:], dtype=np.uint8).reshape(m, 13)
    assert (tris[:, 0] == 3).all()
    return rows[:, :12].copy().view("<f4").reshape(n, 3), rows[:, 12:].copy(), tris[:, 1:].copy().view("<i4").reshape(m, 3)


@pytest.mark.parametrize("n, m", [(0, 0), (3, 1), (500, 977)])
def test_ply_bytes_parse_back(n, m):
    from coponerf_amd.mesh import ply_bytes
    rng = np.random.default_rng(n)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    faces = rng.integers(0, max(n, 1), size=(m, 3)).astype(np.int32)
    back = parse_ply(ply_bytes(xyz, rgb, faces))
    assert back[0].tobytes() == xyz.tobytes() and np.array_equal(back[1], rgb) and np.array_equal(back[2], faces)
    with pytest.raises(ValueError):
        ply_bytes(xyz.astype(np.float64), rgb, faces)
    with pytest.raises(ValueError):
        ply_bytes(xyz, rgb, faces.astype(np.int64))


def test_entry_checks_refuse_host_tensors():
    """Tiny CPU tensors of otherwise valid shape: K = 2 views of a 4 x 4 grid and a 2 x 2 x 2 volume.  No library load."""
    import torch
    from coponerf_amd import mesh
    views = {"depth": torch.ones(2, 1, 16), "valid": torch.ones(2, 1, 16, dtype=torch.uint8), "rgb": torch.zeros(2, 1, 16, 3),
             "poses": torch.eye(4).expand(2, 1, 4, 4).contiguous()}
    with pytest.raises(RuntimeError, match="HIP device only"):
        mesh.integrate(views, torch.eye(4).expand(1, 4, 4).contiguous(), 4, dims=(2, 2, 2), bounds=(torch.zeros(1, 3), torch.ones(1, 3)))
    volume = mesh.Volume(torch.ones(1, 2, 2, 2), torch.zeros(1, 2, 2, 2, dtype=torch.uint8), torch.zeros(1, 2, 2, 2, 3),
                         torch.zeros(1, 3), torch.ones(1, 3), torch.ones(1), (2, 2, 2))
    with pytest.raises(RuntimeError, match="HIP device only"):
        volume.extract()
