"""tests/raster_ref.py, the numpy restatement of csrc/raster.hip that tests/test_gpu_raster.py compares the kernels with EXACTLY, is
pinned here on the CPU against things that do not share its code: a painter's implementation (one face after the other, one pixel
after the other, Python integers and floats, the fill rule as the sign of the edge functions at a centre moved by (e, e^2)), the
watertightness of a sheet, the closedness of a sphere, a plane's closed-form depth.  And every case is held to an empty band:
no floating-point decision of any fixture lies within 1e-9 of its threshold, so nothing is left out of a GPU comparison.
"""
from fractions import Fraction

import numpy as np
import pytest

from coponerf_amd import _hip
from tests import mesh_ref as mr
from tests import raster_ref as rr


def test_the_header_declares_the_entry_points_and_the_threshold():
    assert rr.SMALL == _hip.CONSTANTS["RASTER_SMALL"] and _hip.ABI_VERSION == 12
    assert len(_hip.SIGNATURES["cpn_raster_faces"]) == 16 and len(_hip.SIGNATURES["cpn_raster_resolve"]) == 20


@pytest.mark.parametrize("name", sorted(rr.all_cases()))
def test_every_fixture_has_an_empty_band(name):
    case = rr.all_cases()[name]
    for cull in (0, 1):
        for shade in (0, 1):
            out = rr.draw(case, cull, shade)
            assert not out["band"], (name, cull, shade)
    covered = rr.draw(case)["index"] >= 0
    print(name, "covered pixels", int(covered.sum()), "of", covered.size)
    assert covered.any()


# --------------------------------------------------------------------------------------------------- the painter's implementation
def _sign(E, dx, dy):
    """The sign of an edge function at the pixel centre moved by (e, e^2), e > 0 as small as needed: E + dx e^2 - dy e."""
    key = (E, -dy, dx)
    return 1 if key > (0, 0, 0) else (-1 if key < (0, 0, 0) else 0)


def painter(case, k, b, cull, near=rr.NEAR):
    """(index (H, W), depth (H, W) float32, colour (H, W, 3)) of camera k of pair b: the faces in order, an explicit depth test."""
    H, W = case["H"], case["W"]
    P, Km = case["poses"][k, b].astype(np.float64), case["intrinsics"][b].astype(np.float64)
    nv, nf = min(max(int(case["nvert"][b]), 0), case["capv"]), min(max(int(case["nface"][b]), 0), case["capf"])
    index, depth = np.full((H, W), -1, dtype=np.int64), np.full((H, W), np.inf, dtype=np.float32)
    colour = np.zeros((H, W, 3), dtype=np.uint8)
    for f in range(nf):
        tri = [int(i) for i in case["faces"][b, f]]
        if not all(0 <= i < nv for i in tri):
            continue
        X = case["xyz"][b, tri].astype(np.float64)
        if not np.isfinite(X).all():
            continue
        Y = (X - P[:3, 3]) @ P[:3, :3]                                   # R^T (X - t), row by row
        if not (Y[:, 2] >= near).all():
            continue
        u, v = Km[0, 0] * Y[:, 0] / Y[:, 2] + Km[0, 2], Km[1, 1] * Y[:, 1] / Y[:, 2] + Km[1, 2]
        sx, sy = [int(np.floor(256.0 * a + 0.5)) for a in u], [int(np.floor(256.0 * a + 0.5)) for a in v]
        if max(abs(a) for a in sx + sy) >= 2 ** 29:
            continue
        area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0])
        if area == 0 or (cull and area > 0):
            continue
        col = case["rgb"][b, tri].astype(np.float64)
        for r in range(max(-(-min(sy) // 256), 0), min(max(sy) // 256, H - 1) + 1):
            for c in range(max(-(-min(sx) // 256), 0), min(max(sx) // 256, W - 1) + 1):
                w, signs = [], []
                for a, e in ((1, 2), (2, 0), (0, 1)):
                    dx, dy = sx[e] - sx[a], sy[e] - sy[a]
                    w.append(dx * (256 * r - sy[a]) - dy * (256 * c - sx[a]))
                    signs.append(_sign(w[-1], dx, dy))
                if not (signs == [1, 1, 1] or signs == [-1, -1, -1]):
                    continue
                q = np.array([w[i] / Y[i, 2] for i in range(3)])
                z = np.float32(area / q.sum())
                if z < depth[r, c]:                                      # a later face needs a strictly smaller depth
                    index[r, c], depth[r, c] = f, z
                    colour[r, c] = np.clip(np.floor((q / q.sum()) @ col + 0.5), 0, 255)
    return index, depth, colour


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("name", ["main", "sheet", "lattice", "tilted", "mixed", "sphere"])
def test_against_the_painter(name, cull):
    case = rr.all_cases()[name]
    want = rr.draw(case, cull, 0)
    for k in range(case["K"]):
        for b in range(case["B"]):
            index, depth, colour = painter(case, k, b, cull)
            hit = index >= 0
            assert np.array_equal(want["index"][k, b], index), (name, k, b)
            # the painter sums the face's vertices as stored, the restatement in the canonical order: one fp32 step at the most
            bits = want["bits"][k, b][hit].astype(np.int64)
            assert (np.abs(bits - depth[hit].view(np.uint32).astype(np.int64)) <= 1).all()
            assert np.array_equal(want["frames"][k, b][hit], colour[hit])          # no byte rounding lies in the band
            assert (want["frames"][k, b][~hit] == 0).all()


def test_main_case_holds_what_it_says():
    case = rr.main_case()
    out = rr.draw(case)
    assert (case["K"], case["B"], case["H"], case["W"]) == (3, 2, 40, 48) and list(case["nface"]) == [case["hostile"] + 7, 0]
    assert (out["index"][:, 1] == -1).all() and (out["zbuf"][:, 1] == rr.EMPTY).all()
    assert (out["index"][:, 0] < case["hostile"]).all()                  # no hostile face and no row beyond nface shows
    assert (out["index"][0, 0] >= 0).all()                               # the sheet fills camera 0's image
    s0 = rr.setup(case["xyz"][0], int(case["nvert"][0]), case["faces"][0, :case["nface"][0]], case["poses"][0, 0], case["intrinsics"][0], rr.NEAR)
    s2 = rr.setup(case["xyz"][0], int(case["nvert"][0]), case["faces"][0, :case["nface"][0]], case["poses"][2, 0], case["intrinsics"][0], rr.NEAR)
    assert not s0["ok"][case["hostile"]:].any() and (~s0["ok"][:case["hostile"]]).sum() == 12      # 6 behind, 6 astride
    z2 = s2["cam"][:, :, 2]
    astride = ((z2 < rr.NEAR).any(axis=1) & (z2 >= rr.NEAR).any(axis=1))[:242]
    print("camera 2: sheet faces astride near", int(astride.sum()), "drawn", int(s2["ok"][:242].sum()), "covered", int((out["index"][2, 0] >= 0).sum()))
    assert astride.sum() >= 10 and not s2["ok"][:242][astride].any() and s2["ok"][:242].any() and (out["index"][2, 0] >= 0).any()
    partly = rr.boxes(s0, case["H"], case["W"])
    X, Yc = s0["X"][242:266], s0["Y"][242:266]
    outside = (X.min(axis=1) < 0) | (X.max(axis=1) > 256 * (case["W"] - 1)) | (Yc.min(axis=1) < 0) | (Yc.max(axis=1) > 256 * (case["H"] - 1))
    assert (outside & (partly[2][242:266] > 0)).sum() >= 3               # loose faces partly outside the image


def test_mixed_case_boxes_straddle_the_threshold():
    case = rr.mixed_case()
    s = rr.setup(case["xyz"][0], int(case["nvert"][0]), case["faces"][0], case["poses"][0, 0], case["intrinsics"][0], rr.NEAR)
    _, _, bw, bh = rr.boxes(s, case["H"], case["W"])
    assert s["ok"].all() and np.array_equal(bw * bh, case["boxes"])
    n = bw * bh
    assert {1, rr.SMALL - 1, rr.SMALL, rr.SMALL + 1} <= set(n.tolist()) and (n[list(rr.MIXED_BIG)] == 64 * 64).all()
    for wave in (0, 2):                                                  # a large face and small ones in the same 64 rows
        rows = n[64 * wave:64 * wave + 64]
        assert (rows > rr.SMALL).any() and (rows <= rr.SMALL).any() and (rows == 64 * 64).any()
    index = rr.draw(case)["index"][0, 0]
    assert (index >= 0).all() and np.isin(index, rr.MIXED_BIG).any() and (~np.isin(index, rr.MIXED_BIG)).any()


def test_wide_and_pile_cases_hold_what_they_say():
    wide = rr.draw(rr.wide_case())
    assert rr.wide_case()["capf"] > 70000 and (wide["index"] > 65535).sum() >= 50
    pile = rr.draw(rr.pile_case())["index"][0, 0]
    assert pile[rr.PILE_A[1], rr.PILE_A[0]] == 0 and pile[rr.PILE_B[1], rr.PILE_B[0]] == rr.PILE_N + rr.PILE_SPLIT
    times = rr.draw(rr.pile_case())["times"][0, 0]
    assert times[rr.PILE_A[1], rr.PILE_A[0]] == rr.PILE_N and times[rr.PILE_B[1], rr.PILE_B[0]] == rr.PILE_N and times.sum() == 2 * rr.PILE_N


# ------------------------------------------------------------------------------------------------------------ the fill rule
def test_sheet_is_watertight():
    case = rr.sheet_case()
    out = rr.draw(case)
    assert case["capf"] == 242 and out["times"].shape == (1, 1, 40, 48)
    assert (out["times"] == 1).all()                                     # every pixel: exactly one face, before the depth test


def _on_boundary(case):
    """The pixel centres that lie exactly on an edge or a vertex of a face they are inside of or on: bool (H, W)."""
    H, W = case["H"], case["W"]
    s = rr.setup(case["xyz"][0], int(case["nvert"][0]), case["faces"][0], case["poses"][0, 0], case["intrinsics"][0], rr.NEAR)
    w00, sc, sr, _ = rr.edges(s)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    w = w00[:, None, None, :] + c[None, :, :, None] * sc[:, None, None, :] + r[None, :, :, None] * sr[:, None, None, :]
    return ((w >= 0).all(axis=-1) & (w == 0).any(axis=-1) & s["ok"][:, None, None]).any(axis=0)


def test_shared_edges_and_vertices_have_one_owner_and_index_order_does_not_matter():
    case = rr.lattice_case()
    out = rr.draw(case)
    edge = _on_boundary(case)
    print("lattice: pixel centres on an edge or a vertex", int(edge.sum()), "of", edge.size)
    assert edge.sum() >= 50
    assert (out["times"][0, 0][edge] == 1).all() and (out["times"] == 1).all()
    on_vertex = 0
    for (u, v), colour in zip(case["pixel_uv"], case["rgb"][0]):         # a centre on a vertex shows that vertex's bytes
        if u == int(u) and v == int(v) and 0 <= u < case["W"] and 0 <= v < case["H"]:
            assert np.array_equal(out["frames"][0, 0, int(v), int(u)], colour)
            on_vertex += 1
    assert on_vertex >= 10
    for how in (1, 2, -1):
        other = rr.draw(rr.reindexed(case, how))
        for what in ("zbuf", "index", "bits", "frames", "times"):
            assert np.array_equal(out[what], other[what]), (how, what)
        assert np.array_equal(rr.draw(rr.reindexed(case, how), 0, 1)["frames"], rr.draw(case, 0, 1)["frames"])
        moved = np.roll(other["bary"], -how, axis=-1) if how > 0 else other["bary"][..., ::-1]
        assert np.array_equal(moved.view(np.uint32), out["bary"].view(np.uint32))    # the weights follow their vertices
    main = rr.main_case()                                                # and on the main case, where the depths are not flat
    for how in (1, 2, -1):
        a, b = rr.draw(main), rr.draw(rr.reindexed(main, how))
        assert all(np.array_equal(a[what], b[what]) for what in ("zbuf", "frames"))


# ----------------------------------------------------------------------------------------------------------------- culling
def test_culling_on_a_closed_sphere():
    case = rr.sphere_case()
    xyz, faces = case["xyz"][0], case["faces"][0]
    assert set(mr.edge_counts(faces).values()) == {2}                    # closed
    assert mr.signed_volume(xyz, faces) > 0                              # wound outwards, as cpn_surface_faces winds
    both, front = rr.draw(case, 0), rr.draw(case, 1)
    covered = both["index"] >= 0
    assert covered.reshape(3, -1).sum(axis=1).min() > 150 and not covered[:, :, 0].any() and not covered[:, :, :, 0].any()
    assert np.array_equal(front["index"] >= 0, covered)                  # seen from outside: the front faces cover the same pixels
    assert np.array_equal(front["zbuf"], both["zbuf"])                   # and they are the nearest
    # Every winding reversed.  On a CLOSED surface that cannot draw nothing: the far side's faces now wind towards the camera.
    # What holds: cull = 1 draws none of the faces it drew before, the same pixels (the far side fills the same outline), each
    # strictly deeper; and the side the cameras see, taken alone and reversed, draws nothing at all.
    inside_out = rr.draw(rr.reindexed(case, -1), 1)
    assert np.array_equal(inside_out["index"] >= 0, covered)
    assert not any(np.isin(inside_out["index"][k][covered[k]], front["index"][k][covered[k]]).any() for k in range(3))
    assert (inside_out["bits"][covered] > front["bits"][covered]).all()
    assert np.array_equal(rr.draw(rr.reindexed(case, -1), 0)["zbuf"], both["zbuf"])
    for k in range(3):
        one = rr.near_side(case, k)
        assert 100 < one["kept"] < len(faces) and np.array_equal(rr.draw(one, 1)["zbuf"], front["zbuf"][k:k + 1])
        assert (rr.draw(rr.reindexed(one, -1), 1)["index"] == -1).all()  # nothing faces the camera
        assert np.array_equal(rr.draw(rr.reindexed(one, -1), 0)["zbuf"], front["zbuf"][k:k + 1])


def test_the_sheet_is_wound_away_from_its_camera():
    case = rr.sheet_case()
    assert (rr.draw(case, 1)["index"] == -1).all()
    assert np.array_equal(rr.draw(rr.reindexed(case, -1), 1)["zbuf"], rr.draw(case, 0)["zbuf"])


# ------------------------------------------------------------------------------------------------------- depth, weights, colour
def test_depth_is_the_plane_through_the_snapped_vertices():
    case = rr.tilted_case()
    s = rr.setup(case["xyz"][0], 3, case["faces"][0], case["poses"][0, 0], case["intrinsics"][0], rr.NEAR)
    w00, sc, sr, _ = rr.edges(s)
    X, Y, z = [int(v) for v in s["X"][0]], [int(v) for v in s["Y"][0]], [Fraction(float(v)) for v in s["cam"][0, :, 2]]
    # 1 / z is affine on the screen: solve for it through the three snapped vertices, exactly
    det = Fraction((X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]))
    i0, i1, i2 = 1 / z[0], 1 / z[1], 1 / z[2]
    gx = ((i1 - i0) * (Y[2] - Y[0]) - (i2 - i0) * (Y[1] - Y[0])) / det
    gy = ((i2 - i0) * (X[1] - X[0]) - (i1 - i0) * (X[2] - X[0])) / det
    index = rr.draw(case)["index"][0, 0]
    rows, cols = np.nonzero(index == 0)
    assert len(rows) > 40
    w = w00[0] + cols[:, None] * sc[0] + rows[:, None] * sr[0]
    _, _, z32 = rr._depth(w, s["cam"][:1, :, 2], s["area"][:1])
    q = w.astype(np.float64) / s["cam"][0, :, 2]
    got = s["area"][0].astype(np.float64) / ((q[:, 0] + q[:, 1]) + q[:, 2])
    for r, c, g, g32 in zip(rows, cols, got, z32):
        want = 1 / (i0 + gx * (256 * int(c) - X[0]) + gy * (256 * int(r) - Y[0]))
        assert abs(Fraction(float(g)) - want) <= Fraction(1, 10 ** 12) * want
        assert np.float32(float(want)) == g32 or abs(Fraction(float(g32)) - want) <= Fraction(1, 2 ** 23) * want
    assert np.array_equal(rr.draw(case)["bits"][0, 0][rows, cols], z32.view(np.uint32))


def test_weights_sum_to_one_and_corners_show_their_bytes():
    for case in (rr.main_case(), rr.tilted_case(), rr.sphere_case()):
        out = rr.draw(case)
        hit = out["index"] >= 0
        total = out["bary"][hit].astype(np.float64).sum(axis=-1)
        assert (np.abs(total - 1.0) <= 2 * 2.0 ** -23).all() and (out["bary"][hit] >= 0).all()
        assert np.isnan(out["bary"][~hit]).all()
    case = rr.tilted_case()                                              # a key naming the face at the two pixels on vertices
    zbuf = np.full((1, 1, case["H"], case["W"]), rr.EMPTY, dtype=np.uint64)
    for c, r in case["corners"]:
        zbuf[0, 0, r, c] = np.uint64(0x40000000) << np.uint64(32)
    out = rr.resolve(zbuf, case, case["poses"], case["intrinsics"])
    for vertex, (c, r) in enumerate(case["corners"]):
        assert np.array_equal(out["frames"][0, 0, r, c], case["rgb"][0, vertex])
        assert np.array_equal(out["bary"][0, 0, r, c], np.eye(3, dtype=np.float32)[vertex])
    assert (out["index"] >= 0).sum() == 2


def test_headlight_is_brightest_where_the_surface_faces_the_camera():
    case = rr.sphere_case()
    out = rr.draw(case, 0, 1)
    grey = out["frames"][0, 0].astype(np.int64)
    hit = out["index"][0, 0] >= 0
    assert (grey[..., 0] == grey[..., 1]).all() and (grey[..., 1] == grey[..., 2]).all()
    r, c = np.nonzero(hit)
    centre = (r - r.mean()) ** 2 + (c - c.mean()) ** 2 < 9
    rim = (r - r.mean()) ** 2 + (c - c.mean()) ** 2 > 49
    assert grey[r[centre], c[centre], 0].min() > 200 and grey[r[rim], c[rim], 0].mean() < grey[r[centre], c[centre], 0].mean() - 40


def test_entry_checks_refuse_host_tensors():
    """Tiny CPU tensors of otherwise valid shape: one triangle, one camera, H = W = 4.  No library load."""
    import torch
    from coponerf_amd import raster
    from coponerf_amd.mesh import Mesh
    one = torch.ones(1, dtype=torch.int32)
    mesh = Mesh(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3, dtype=torch.uint8), 3 * one, torch.tensor([[[0, 1, 2]]], dtype=torch.int32), one)
    poses, intr = torch.eye(4).expand(1, 1, 4, 4).contiguous(), torch.eye(4).expand(1, 4, 4).contiguous()
    with pytest.raises(RuntimeError, match="HIP device only"):
        raster.raster_faces(mesh, poses, intr, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        raster.resolve(torch.full((1, 1, 4, 4), -1, dtype=torch.int64), mesh, poses, intr)
