"""coponerf_amd.matches on the MI355X (`pytest -m gpu`): the kernels of csrc/matches.hip element by element against the restatements
of tests/matches_ref.py (pinned on the CPU by tests/test_matches_ref.py), and from_pair end to end.

Every output buffer starts as NaN (floats) or 0xFF (bytes, counts) between guard rows; nothing is left out of a comparison
except the mask decisions inside the 1e-3 px band of a threshold, which are counted and held to 0.5 % of the pixels.  The
bounds are tests/matches_ref.py's, from operation counts; compacted bytes, counts and statuses exactly.
"""
import warnings

import numpy as np
import pytest
import torch

from coponerf_amd import _hip, synthetic as syn
from tests import matches_ref as mr
from tests.test_gpu_point_cloud import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG = _hip.CONSTANTS["E_SHAPE"], _hip.CONSTANTS["E_ARG"]
TILE = _hip.CONSTANTS["COMPACT_TILE"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------ match fields
def _run_fields(B, S, h, dev):
    f0, f1, K, P = (_up(a, dev) for a in mr.fields_case(B, S, h))
    n = 2 * B * S * S
    q, cycle, epi, inside = (Guarded(2 * n, torch.float32, dev), Guarded(n, torch.float32, dev), Guarded(n, torch.float32, dev),
                             Guarded(n, torch.uint8, dev))
    _hip.call("cpn_match_fields", f0.data_ptr(), f1.data_ptr(), K.data_ptr(), P.data_ptr(), B, S, h, q.ptr, cycle.ptr, epi.ptr,
              inside.ptr, _hip.stream_handle())
    return (q.get().reshape(2, B, S, S, 2), cycle.get().reshape(2, B, S, S), epi.get().reshape(2, B, S, S),
            inside.get().reshape(2, B, S, S))


@pytest.mark.parametrize("B,S,h", ((2, 32, 8), (2, 24, 8)))
def test_match_fields_against_float64(dev, B, S, h):
    _, _, K, P = mr.fields_case(B, S, h)
    ref = mr.fields_ref(B, S, h)
    q, cycle, epi, inside = _run_fields(B, S, h, dev)
    assert set(np.unique(inside)) <= {0, 1}                        # every element written, none left 0xFF

    assert np.array_equal(np.isnan(q), np.isnan(ref["q"]))
    ok = ~np.isnan(ref["q"])
    ratio = (np.abs(q.astype(np.float64) - ref["q"])[ok] / ref["q_bound"][ok]).max()
    print(S, "q: largest error / bound", float(ratio), "; bits equal to the fp32 restatement:", q.tobytes() == ref["q32"].tobytes())
    assert ratio <= 1.0

    assert np.array_equal(np.isnan(cycle), np.isnan(ref["cycle"])) and np.array_equal(np.isinf(cycle), np.isinf(ref["cycle"]))
    ok = np.isfinite(ref["cycle"])
    ratio = (np.abs(cycle.astype(np.float64) - ref["cycle"])[ok] / ref["cycle_bound"][ok]).max()
    print(S, "cycle: largest error / bound", float(ratio), "of", int(ok.sum()), "finite,", int((~ok).sum()), "not")
    assert ratio <= 1.0 and (~ok).sum() > 0

    # inside is decided on the fp32 match the kernel wrote: exactly, every pixel; against the float64 match outside the band
    with np.errstate(invalid="ignore"):
        own = (q[..., 0] >= 0) & (q[..., 0] <= S - 1) & (q[..., 1] >= 0) & (q[..., 1] <= S - 1)
        got_mask = (cycle <= 10.0) & (inside != 0)
    assert np.array_equal(inside != 0, own)
    mask, far = mr.mask_of(ref)
    print(S, "pixels in the band", int((~far).sum()), "of", far.size, "; mask share", float(mask.mean()))
    assert (~far).sum() <= mr.BAND_SHARE * far.size
    assert np.array_equal((inside != 0)[far], ref["inside"][far]) and np.array_equal(got_mask[far], mask[far])

    want, bound = mr.epi_field(q, K, P)                            # float64 from the kernel's own fp32 matches, one rounding
    assert np.array_equal(np.isnan(epi), np.isnan(want))
    ok = ~np.isnan(want)
    ratio = (np.abs(epi.astype(np.float64) - want)[ok] / bound[ok]).max()
    print(S, "epi: largest error / bound", float(ratio), "of", int(ok.sum()), "; NaN", int((~ok).sum()))
    assert ratio <= 1.0 and ok.sum() > 0.9 * ok.size and (~ok).sum() > 0


def test_mask_against_stock_cycle_masks_on_the_device(dev):
    """S = 256, h = 64, the reference's sizes: (cycle <= 10) & inside of the kernel is aux_outputs.cycle_masks' stock-op chain on
    the device, outside the band."""
    from coponerf_amd.aux_outputs import cycle_masks
    B, S, h = 2, 256, 64
    f0, f1, _, _ = mr.fields_case(B, S, h)
    _, far = mr.mask_of(mr.fields_ref(B, S, h))
    _, cycle, _, inside = _run_fields(B, S, h, dev)
    m1, m2 = cycle_masks((_up(f0, dev), _up(f1, dev)), h)
    stock = np.stack((m1.cpu().numpy().astype(bool), m2.cpu().numpy().astype(bool)))
    with np.errstate(invalid="ignore"):
        got = (cycle <= 10.0) & (inside != 0)
    print("band", int((~far).sum()), "of", far.size, "; differing inside it", int((got != stock)[~far].sum()), "; mask share", float(got.mean()))
    assert (~far).sum() <= mr.BAND_SHARE * far.size and 0.2 <= got.mean() <= 0.75
    assert np.array_equal(got[far], stock[far])


def test_bad_shapes_are_status_codes(dev):
    """Shapes the kernels do not take come back as status codes before any launch (the pointers are one small valid buffer)."""
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    for B, S, h in ((0, 32, 8), (1, 30, 8), (1, 32, 0), (1, 32768, 8), (32768, 8, 8)):
        assert lib.cpn_match_fields(p, p, p, p, B, S, h, p, p, p, p, s) == E_SHAPE
        assert b"cpn_match_fields" in lib.cpn_last_error()
    for B, S in ((0, 32), (1, 0), (40000, 8), (600, 2048)):
        assert lib.cpn_compact_matches(p, p, p, p, B, S, p, p, p, p, s) == E_SHAPE
        assert lib.cpn_compact_matches_scratch(B, S) == 0
    assert lib.cpn_refine_pose(p, p, p, p, 0, 8, 1, 2.0, p, p, s) == E_SHAPE
    assert lib.cpn_refine_pose(p, p, p, p, 1, 0, 1, 2.0, p, p, s) == E_SHAPE
    assert lib.cpn_refine_pose(p, p, p, p, 1, 8, -1, 2.0, p, p, s) == E_ARG
    assert lib.cpn_refine_pose(p, p, p, p, 1, 8, 1, 0.0, p, p, s) == E_ARG
    assert lib.cpn_refine_pose(p, p, p, p, 1, 8, 1, float("nan"), p, p, s) == E_ARG
    assert lib.cpn_match_fields(0, p, p, p, 1, 32, 8, p, p, p, p, s) == E_ARG
    torch.cuda.synchronize()
    assert not bool(buf.any())                                   # nothing ran


# -------------------------------------------------------------------------------------------------------------- compaction
def _run_compact(keep, q, cycle, epi, dev):
    _, B, S, _ = keep.shape
    cap = 2 * S * S
    kd, qd, cd, ed = (_up(a, dev) for a in (keep, q, cycle, epi))
    n_scratch = _hip.lib().cpn_compact_matches_scratch(B, S)
    assert n_scratch == B * -(-cap // TILE)
    scratch = torch.empty(n_scratch, dtype=torch.int32, device=dev)
    xy, err, count = Guarded(B * cap * 4, torch.float32, dev), Guarded(B * cap * 2, torch.float32, dev), Guarded(B, torch.int32, dev)
    _hip.call("cpn_compact_matches", kd.data_ptr(), qd.data_ptr(), cd.data_ptr(), ed.data_ptr(), B, S, scratch.data_ptr(), xy.ptr,
              err.ptr, count.ptr, _hip.stream_handle())
    return xy.get().reshape(B, cap, 4), err.get().reshape(B, cap, 2), count.get()


def _check_compact(keep, q, cycle, epi, dev):
    want_xy, want_err, want_n = mr.compact(keep, q, cycle, epi)
    got = _run_compact(keep, q, cycle, epi, dev)
    assert np.array_equal(got[2], want_n)
    for b in range(keep.shape[1]):
        n = int(want_n[b])
        assert got[0][b, :n].tobytes() == want_xy[b].tobytes() and got[1][b, :n].tobytes() == want_err[b].tobytes()
        assert np.isnan(got[0][b, n:]).all() and np.isnan(got[1][b, n:]).all()      # rows beyond the count: untouched
    again = _run_compact(keep, q, cycle, epi, dev)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))               # two runs, the same bytes
    return want_n


def _compact_inputs(B, S, seed):
    """Distinct finite values everywhere (a NaN would look like an untouched row) except one NaN epi that is never kept."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-5, S + 5, size=(2, B, S, S, 2)).astype(np.float32)
    cycle = rng.uniform(0, 20, size=(2, B, S, S)).astype(np.float32)
    epi = rng.normal(size=(2, B, S, S)).astype(np.float32)
    return q, cycle, epi


def test_compact_the_fields_selection_and_the_two_ends(dev):
    B, S, h = 2, 32, 8
    ref = mr.fields_ref(B, S, h, False)
    mask, _ = mr.mask_of(ref)
    q, cycle = ref["q32"], ref["cycle"].astype(np.float32)
    epi = np.nan_to_num(ref["epi"].astype(np.float32), nan=0.0)
    keep = mask.astype(np.uint8) * 3                              # any non-zero byte selects
    n = _check_compact(keep, q, cycle, epi, dev)
    assert (n > 0.2 * 2 * S * S).all() and (n < 0.75 * 2 * S * S).all()
    assert (_check_compact(np.ones_like(keep), q, cycle, epi, dev) == 2 * S * S).all()
    assert (_check_compact(np.zeros_like(keep), q, cycle, epi, dev) == 0).all()


@pytest.mark.parametrize("kept", (TILE, TILE + 1))
def test_compact_counts_at_the_tile_edge(dev, kept):
    """One pair of 2 . 32 . 32 = 2 048 elements, two workgroups: the first CPN_COMPACT_TILE kept fill the first workgroup's tile
    exactly, one more is the second workgroup's first; and the same number scattered over both directions."""
    B, S = 1, 32
    q, cycle, epi = _compact_inputs(B, S, 16)
    keep = np.zeros((2, B, S, S), dtype=np.uint8)
    keep.reshape(-1)[:kept] = 1
    assert _check_compact(keep, q, cycle, epi, dev)[0] == kept
    rng = np.random.default_rng(kept)
    keep = np.zeros(2 * S * S, dtype=np.uint8)
    keep[rng.permutation(2 * S * S)[:kept]] = 255
    assert _check_compact(keep.reshape(2, B, S, S), q, cycle, epi, dev)[0] == kept


def test_compact_three_pairs_with_different_counts(dev):
    """B = 3, S = 24: 1 152 elements per pair, the second tile is partly beyond the sequence; pair 1 keeps nothing."""
    B, S = 3, 24
    q, cycle, epi = _compact_inputs(B, S, 17)
    rng = np.random.default_rng(18)
    keep = (rng.random((2, B, S, S)) < np.array([0.15, 0.0, 0.9])[None, :, None, None]).astype(np.uint8)
    n = _check_compact(keep, q, cycle, epi, dev)
    assert n[1] == 0 and 0 < n[0] < n[2] < 2 * S * S


# -------------------------------------------------------------------------------------------------------------- refinement
N = 1000
COUNTS = (1000, 0, 7)


def _batch(scene, counts=COUNTS, poses=None):
    """B = 3 pairs of N = 1000 rows: the scene's matches up to the pair's count, NaN beyond."""
    B = len(counts)
    xy = np.full((B, N, 4), np.nan, dtype=np.float32)
    for b, c in enumerate(counts):
        xy[b, :c] = scene["xy"][:c]
    K = np.stack([scene["intrinsics"]] * B)
    P = np.stack([scene["rel_pose"]] * B) if poses is None else np.stack(poses)
    return xy, np.asarray(counts, dtype=np.int32), K.astype(np.float32), P.astype(np.float32)


def _run_refine(xy, count, K, P, iters, scale, dev):
    B, n = xy.shape[:2]
    xd, cd, kd, pd = (_up(a, dev) for a in (xy, count, K, P))
    pose, stats = Guarded(B * 16, torch.float32, dev), Guarded(B * 8, torch.float64, dev)
    _hip.call("cpn_refine_pose", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), pd.data_ptr(), B, n, iters, scale, pose.ptr, stats.ptr,
              _hip.stream_handle())
    return pose.get().reshape(B, 4, 4), stats.get().reshape(B, 8)


def _refine_checked(batch, iters, dev, scale=2.0):
    """The conditions every refinement case meets: two runs give the same bytes, a pair's result is the same alone and in the
    batch, a pair without matches returns rel_pose's bits with status 2.  -> (pose, stats, the reference's per pair)."""
    xy, count, K, P = batch
    pose, stats = _run_refine(xy, count, K, P, iters, scale, dev)
    again = _run_refine(xy, count, K, P, iters, scale, dev)
    assert pose.tobytes() == again[0].tobytes() and stats.tobytes() == again[1].tobytes()
    refs = []
    for b in range(len(count)):
        alone = _run_refine(xy[b:b + 1], count[b:b + 1], K[b:b + 1], P[b:b + 1], iters, scale, dev)
        assert alone[0][0].tobytes() == pose[b].tobytes() and alone[1][0].tobytes() == stats[b].tobytes(), b
        refs.append(mr.refine_pose(xy[b], count[b], K[b], P[b], iters, scale))
        assert stats[b, 7] == refs[b][1][7] and stats[b, 6] == refs[b][1][6] and stats[b, 3] == refs[b][1][3], (b, stats[b], refs[b][1])
        if count[b] == 0:
            assert pose[b].tobytes() == P[b].tobytes() and stats[b, 7] == 2 and not stats[b, :7].any()
    assert (np.isfinite(pose) | ~np.isfinite(P)).all()              # never a NaN pose out of a finite one
    assert (pose[:, 3] == np.array([0, 0, 0, 1], dtype=np.float32)).all()
    return pose, stats, refs


def test_refine_one_step_against_the_reference(dev):
    """iters = 1: every entry of the pose within half an fp32 ulp plus refine_step_bound (operation count, sums of absolute
    terms of H and g, cond(A)) of the reference's single step; the sums of the statistics within their own operation counts.
    Observed on the MI355X: the largest error is 0.18 of the bound for the pair of 1 000 matches (cond(A) 1.2e3, step bound
    1.6e-7) and 0.37 for the pair of 7 (cond(A) 1.2e4, step bound 5.1e-8); both poses ARE the reference's rounded to fp32, so
    what is left is the store's half ulp."""
    sc = mr.refine_scene()
    batch = _batch(sc)
    pose, stats, refs = _refine_checked(batch, 1, dev)
    len0 = float(np.linalg.norm(sc["rel_pose"][:3, 3].astype(np.float64)))
    for b in (0, 2):
        want, wstats, trace = refs[b]
        d_delta, b_rot, b_tr, cond = mr.refine_step_bound(trace[0], 2.0, len0)
        bound = np.zeros((4, 4))
        bound[:3, :3], bound[:3, 3] = b_rot, b_tr
        bound += mr.half_ulp32(want)
        err = np.abs(pose[b].astype(np.float64) - want)
        exact = np.abs(pose[b].astype(np.float64) - want.astype(np.float32).astype(np.float64)).max()
        print("pair", b, "one step: largest error / bound", float((err[:3] / bound[:3]).max()), "cond(A)", cond, "step bound", b_rot,
              "; distance from the reference rounded to fp32", exact)
        assert (err <= bound).all()
        rounds = -(-int(batch[1][b]) // mr.NT)
        rel = (mr.TERM_OPS + rounds + 8) * mr.E                  # a cost or weight term and the depth of its sum; all terms >= 0
        assert abs(stats[b, 0] - wstats[0]) <= rel * wstats[0] and abs(stats[b, 2] - wstats[2]) <= rel * wstats[2]
        # the cost after the step is formed at the updated state, which may differ by d_delta: the cost's gradient is
        # g = sum w r J (d cost / d r = w r), at most the sum of its absolute terms there; twice that covers the second order
        last = trace[-1]
        absg = mr.pass_sums(last["rows"], *last["cams"], last["R"], last["t"], 2.0, magnitude=True)[21:27]
        assert abs(stats[b, 1] - wstats[1]) <= rel * wstats[1] + 2.0 * np.linalg.norm(absg) * d_delta
        assert np.abs(stats[b, 4:6] - wstats[4:6]).max() <= np.degrees(2 * 3 * (b_rot + mr.POSE_OPS * mr.E))
        assert stats[b, 6] == 1 and stats[b, 7] == 0


def test_refine_recovers_the_pose_from_exact_correspondences(dev):
    """iters = 10 on exact correspondences started 5 and 17 degrees off: the device and the reference are each within 1e-4
    degrees of the truth in rotation and in the translation's direction."""
    sc = mr.refine_scene()
    pose, stats, refs = _refine_checked(_batch(sc), 10, dev)
    got, want = mr.pose_errors(pose[0], sc), mr.pose_errors(refs[0][0], sc)
    print("device", got, "reference", want, "stats", stats[0])
    assert max(got) <= 1e-4 and max(want) <= 1e-4
    assert stats[0, 6] == 10 and stats[0, 7] == 0 and stats[0, 3] == 1000 and stats[0, 1] < 1e-6 * stats[0, 0]
    assert abs(stats[0, 4] - 5.0) < 1e-3 and abs(stats[0, 5] - 17.0) < 1e-3
    assert abs(np.linalg.norm(pose[0, :3, 3].astype(np.float64)) - np.linalg.norm(sc["rel_pose"][:3, 3].astype(np.float64))) < 2e-7


def test_refine_underdetermined_pairs(dev):
    """One match and five: the damping and the gauge keep the solve finite, as in the reference (status and updates equal,
    _refine_checked); also with N = 1 and N = 5 rows in all."""
    sc = mr.refine_scene()
    pose, stats, refs = _refine_checked(_batch(sc, counts=(1, 0, 5)), 10, dev)
    for b in (0, 2):
        print("pair", b, "stats", stats[b], "largest distance from the reference", float(np.abs(pose[b] - refs[b][0]).max()))
        assert np.isfinite(pose[b]).all() and np.isfinite(stats[b]).all() and stats[b, 1] <= stats[b, 0]
    xy, _, K, P = _batch(sc)
    for n in (1, 5):
        p, s = _run_refine(xy[:1, :n], np.asarray([n], dtype=np.int32), K[:1], P[:1], 10, 2.0, dev)
        ref = mr.refine_pose(xy[0, :n], n, K[0], P[0], 10, 2.0)
        assert np.isfinite(p).all() and s[0, 7] == ref[1][7] and s[0, 6] == ref[1][6] and s[0, 3] == n
        assert p.tobytes() == pose[0 if n == 1 else 2][None].tobytes()           # rows beyond the count never mattered


def test_refine_nothing_to_do(dev):
    """|t0| = 0, a NaN pose and iters = 0: status 2 and rel_pose's own bits; a count beyond N is N, a negative one 0."""
    sc = mr.refine_scene()
    zero_t, nan_pose = sc["rel_pose"].copy(), sc["rel_pose"].copy()
    zero_t[:3, 3] = 0
    nan_pose[2, 0] = np.nan
    batch = _batch(sc, counts=(1000, 1000, 7), poses=(zero_t, nan_pose, sc["rel_pose"]))
    pose, stats, _ = _refine_checked(batch, 3, dev)
    assert (stats[:2, 7] == 2).all() and not stats[:2, :7].any() and stats[2, 7] == 0
    assert pose[:2].tobytes() == batch[3][:2].tobytes()
    pose, stats, _ = _refine_checked(_batch(sc), 0, dev)
    assert (stats[:, 7] == 2).all() and pose.tobytes() == _batch(sc)[3].tobytes()
    xy, _, K, P = _batch(sc, counts=(1000, 1000, 1000))
    over = _run_refine(xy, np.asarray([1000, 5000, -3], dtype=np.int32), K, P, 2, 2.0, dev)
    assert over[0][1].tobytes() == over[0][0].tobytes() and over[1][2, 7] == 2


# ------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def pair(dev):
    """The synthetic-weight model of the other GPU tests and one pair of 256 x 455 noise photos."""
    from coponerf_amd import CoPoNeRF
    from coponerf_amd.novel_views import prepare_pair
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    return model, prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)


def test_from_pair_end_to_end(dev, pair):
    from coponerf_amd import matches as mt
    model, inp = pair
    S = 256
    first = mt.from_pair(model, inp, max_cycle_px=1e9)            # warms up; the synthetic flows carry no geometry: keep what is inside
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                       # nothing is read on the host
    try:
        res = mt.from_pair(model, inp, max_cycle_px=1e9)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert set(res) == {"matches", "rel_pose", "pose", "stats", "fields"}
    m, f = res["matches"], res["fields"]
    cap = 2 * S * S
    for name, t, shape, dtype in (("xy", m.xy, (1, cap, 4), torch.float32), ("err", m.err, (1, cap, 2), torch.float32),
                                  ("count", m.count, (1,), torch.int32), ("rel_pose", res["rel_pose"], (1, 4, 4), torch.float32),
                                  ("pose", res["pose"], (1, 4, 4), torch.float32), ("stats", res["stats"], (1, 8), torch.float64),
                                  ("q", f["q"], (2, 1, S, S, 2), torch.float32), ("cycle", f["cycle"], (2, 1, S, S), torch.float32),
                                  ("epi", f["epi"], (2, 1, S, S), torch.float32), ("inside", f["inside"], (2, 1, S, S), torch.uint8)):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device == dev, name
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            xy, err = m.numpy(0)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert len([c for c in caught if "synchroniz" in str(c.message)]) == 1      # one read
    n = int(m.count[0])
    assert xy.shape == (n, 4) and err.shape == (n, 2) and xy.dtype == err.dtype == np.float32
    # the selection is the reference's of the fields: inside, one pixel per 4 x 4 cell, in (direction, row, column) order
    with np.errstate(invalid="ignore"):
        keep = mr.stride_keep((f["inside"].cpu().numpy() != 0) & (f["cycle"].cpu().numpy() <= 1e9), 4).astype(np.uint8)
    want = mr.compact(keep, f["q"].cpu().numpy(), f["cycle"].cpu().numpy(), f["epi"].cpu().numpy())
    print("kept", n, "of", cap, "; stats", res["stats"][0].cpu().numpy())
    assert n == want[2][0] and xy.tobytes() == want[0][0].tobytes() and err.tobytes() == want[1][0].tobytes()
    with torch.no_grad():
        assert torch.equal(res["rel_pose"], model.get_z(inp)[1])
    stats = res["stats"][0].cpu().numpy()
    assert np.isfinite(res["pose"].cpu().numpy()).all() and stats[7] in (0.0, 1.0, 2.0) and (n == 0 or stats[7] != 2)
    # a second call gives equal bytes
    xy1, err1 = first["matches"].numpy(0)
    assert xy1.tobytes() == xy.tobytes() and err1.tobytes() == err.tobytes()
    assert torch.equal(first["pose"], res["pose"]) and first["stats"].cpu().numpy().tobytes() == res["stats"].cpu().numpy().tobytes()
    for k in f:
        assert first["fields"][k].cpu().numpy().tobytes() == f[k].cpu().numpy().tobytes(), k
    # refine=False leaves the pose out; the default selection is cycle_masks' own mask on the strided pixels
    plain = mt.from_pair(model, inp, refine=False)
    assert plain["pose"] is None and plain["stats"] is None
    with np.errstate(invalid="ignore"):
        keep10 = mr.stride_keep((f["inside"].cpu().numpy() != 0) & (f["cycle"].cpu().numpy() <= 10.0), 4)
    assert int(plain["matches"].count[0]) == int(keep10.sum())
