"""Yardstick of coponerf_amd.matches.ransac_pose(score="msac", lo=K) (csrc/ransac.hip, round 24 of include/coponerf_hip.h): a numpy
restatement, for ONE pair, of cpn_ransac_score_slots, cpn_ransac_polish and cpn_ransac_finish_lo in the header's operation
sequence.  tests/test_lo_msac_ref.py pins it on the CPU; tests/test_gpu_lo_msac.py compares the kernels with it.

It is built from the restatements the earlier rounds pinned: the residual, the split, the vote and the finish are
tests/ransac_ref.py's, the Gauss-Newton pass, the damping, the solve and the rotation step tests/matches_ref.py's, the 5-point
hypotheses tests/ransac5_ref.py's.  New here: the weight with its floor and clamp, the int64 sums, the rank (the kernel's one sweep with a sorted chain per thread), the polish that joins
the parts, E's write-out and the finish over the hypotheses and the polished slots.

Decisions are integers or comparisons of float64 values both sides form in the same sequence, so they are compared exactly, after
the fixtures have been shown to keep every |r| at least rr.MARGIN = 1e-9 px from the threshold and every weight's value before the
floor at least FLOOR_MARGIN from an integer (floor_margin says which values need no margin): two float64 evaluations of 2^20 (1 - r^2 / px^2) differ by at most about
2^20 x 16 x 2^-53 = 2e-9 (the residual's operations on a quotient below 1), far below FLOOR_MARGIN = 1e-6.
"""
import functools

import numpy as np

from tests import matches_ref as mr
from tests import ransac5_ref as r5
from tests import ransac_ref as rr

ONE = 1 << 20
LO_MAX = 16
CHUNK = rr.CHUNK
FLOOR_MARGIN = 1e-6
BLOCK = 512                                                         # slots per block of the residual table: memory, not arithmetic


# ------------------------------------------------------------------------------------------------------------- the score
def residual_table(Em, valid, xy, intrinsics):
    """(r (H, n) float64, counts (H, n) bool) of the rows xy (n, 4) under the VALID slots of Em (H, 9); invalid slots count
    nowhere.  rr.residuals in blocks of slots."""
    Em, on = np.asarray(Em, dtype=np.float64).reshape(-1, 9), np.asarray(valid) != 0
    r, ok = np.zeros((len(Em), len(xy))), np.zeros((len(Em), len(xy)), dtype=bool)
    idx = np.flatnonzero(on)
    for at in range(0, len(idx), BLOCK):
        sel = idx[at:at + BLOCK]
        r[sel], ok[sel] = rr.residuals(Em[sel], xy, intrinsics)
    return r, ok


def weights(r, ok, inlier_px, defect=None):
    """-> (inlier (H, n) bool, w (H, n) int64, v the values before the floor, NaN where there is no floor to take).
    defect="round": the nearest integer in place of the floor."""
    with np.errstate(all="ignore"):
        inl = ok & (np.abs(r) <= inlier_px)
        if inlier_px > 0.0:
            v = ONE * (1.0 - (r * r) / (inlier_px * inlier_px))
            f = np.floor(v + 0.5) if defect == "round" else np.floor(v)
            w = np.where(f >= ONE, ONE, np.where(f > 0.0, f, 0.0))   # not a number: 0
        else:
            v, w = np.full(r.shape, np.nan), np.full(r.shape, float(ONE))
    return inl, np.where(inl, w, 0.0).astype(np.int64), np.where(inl, v, np.nan)


def floor_margin(v, r, inlier_px):
    """The smallest distance of a value before the floor from an integer (inf where there is none).  A match with
    |r| <= 1e-10 inlier_px - one of the slot's own sample, its residual the elimination's rounding - is left out: its quotient
    lies below 1e-20, 1 - q IS 1 in float64 whatever the last bits of r, and the value is 2^20 exactly in any evaluation."""
    with np.errstate(invalid="ignore"):
        exempt = np.abs(r) <= 1e-10 * inlier_px
    assert (v[exempt & np.isfinite(v)] == ONE).all()
    v = v[np.isfinite(v) & ~exempt]
    return float(np.abs(v - np.rint(v)).min()) if len(v) else np.inf


def chunk_sums(per_row, N, n):
    """per_row (H, n) integers -> (chunks, H) int32: the sums over the chunks of CHUNK rows, zeros at and beyond n."""
    H = len(per_row)
    chunks = -(-N // CHUNK)
    padded = np.zeros((H, chunks * CHUNK), dtype=np.int64)
    padded[:, :n] = per_row
    out = padded.reshape(H, chunks, CHUNK).sum(axis=2).T
    assert out.max(initial=0) <= 2 ** 28
    return np.ascontiguousarray(out.astype(np.int32))


def score(Em, valid, xy, count, intrinsics, inlier_px, graded, rel_pose=None, defect=None):
    """The rule of cpn_ransac_score_slots with first = 0 and total = Hn for one pair -> partial (chunks, Hn + 1) int32: the
    inlier counts (graded False: rr.score's) or the sums of weights; rel_pose's slot last."""
    xy = np.asarray(xy, dtype=np.float32)
    N, Hn = len(xy), len(Em)
    n = min(max(int(count), 0), N)
    slots, on = np.zeros((Hn + 1, 9)), np.zeros(Hn + 1, dtype=bool)
    slots[:Hn], on[:Hn] = Em, np.asarray(valid) != 0
    if rel_pose is not None:
        slots[Hn], on[Hn] = rr.rel_essential(rel_pose), True
    r, ok = residual_table(slots, on, xy[:n], intrinsics)
    inl, w, _ = weights(r, ok, inlier_px, defect)
    return chunk_sums(w if graded else inl, N, n)


# -------------------------------------------------------------------------------------------------------------- the rank
RANK_DEPTH, THREADS = LO_MAX, 256


def ranks_before(a, b, defect=None):
    """(score, slot) a comes before b in (score descending, slot ascending) order; slot -1 is "none" and comes last.
    defect="last on ties": the higher slot first."""
    if a[1] < 0:
        return False
    return b[1] < 0 or a[0] > b[0] or (a[0] == b[0] and (a[1] > b[1] if defect == "last on ties" else a[1] < b[1]))


def ranked_slot(sums, ok, want, defect=None):
    """csrc/ransac_common.h's ranked_slot: thread t keeps the RANK_DEPTH best of its slots t, t + 256, .. sorted (a chain of
    compare-and-swaps), then want + 1 times the workgroup takes the first of the threads' heads - the largest score, then its
    lowest slot - and the thread that held it moves its chain up -> (score, slot) of the one taken last, slot -1 where there is
    none.  defect="last on ties"; defect="skips a slot": the thread that held the head moves its chain up by two."""
    tops = [[(0, -1)] * RANK_DEPTH for _ in range(THREADS)]
    for h in range(len(sums)):
        if not ok[h]:
            continue
        new, top = (int(sums[h]), h), tops[h % THREADS]
        for j in range(RANK_DEPTH):
            if ranks_before(new, top[j], defect):
                new, top[j] = top[j], new
    got = (0, -1)
    for _ in range(want + 1):
        heads = [t[0] for t in tops if t[0][1] >= 0]
        if not heads:
            return 0, -1
        best = max(s for s, _ in heads)
        tied = [h for s, h in heads if s == best]
        got = (best, max(tied) if defect == "last on ties" else min(tied))
        top = tops[got[1] % THREADS]
        del top[:2 if defect == "skips a slot" else 1]
        top += [(0, -1)] * (RANK_DEPTH - len(top))
    return got


def rank_list(sums, valid, K, usable=8, defect=None):
    """The slots of rank 0 .. K - 1 (-1 beyond the valid ones, and everywhere with fewer than 8 usable matches): workgroup
    (k, b)'s ranked_slot with want = k."""
    ok = np.asarray(valid) != 0
    return [ranked_slot(sums, ok, k, defect)[1] if usable >= 8 else -1 for k in range(K)]


# ------------------------------------------------------------------------------------------------------------ the polish
def unit_essential(e):
    """e (9) / |e|_F with the first largest |e_c| positive (csrc/epipolar_system.h) -> (e, every entry finite)."""
    with np.errstate(all="ignore"):
        ss = e[0] * e[0]
        for c in range(1, 9):
            ss = ss + e[c] * e[c]
        e = e / np.sqrt(ss)
        mag = np.where(np.isnan(e), -1.0, np.abs(e))
        if e[int(mag.argmax())] < 0.0:
            e = -e
    return e, bool(np.isfinite(e).all())


def polish(e, xy, count, intrinsics, inlier_px, iters, scale_px, defect=None):
    """One workgroup of cpn_ransac_polish past its rank: the split of e (9), the vote of its inliers, `iters` passes of
    cpn_refine_pose's Gauss-Newton from the picked pose over all rows below n, E = [t]x R normalised and signed
    -> (E (9), valid, info): info = {votes, pick, done, status, R, t, sigma}.  defect="no vote": candidate (R1, +t) always."""
    xy = np.asarray(xy, dtype=np.float32)
    n = min(max(int(count), 0), len(xy))
    R1, R2, t, sigma = rr.split(e)
    if not (np.isfinite(R1).all() and np.isfinite(R2).all() and np.isfinite(t).all()):
        return np.zeros(9), False, {"votes": np.zeros(4, dtype=np.int64), "done": 0, "status": 3}
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    inl = rr.inliers(np.asarray(e)[None], xy[:n], intrinsics, inlier_px)[0]
    v, small = rr.votes(R1, R2, t, tuple(p[inl] for p in rr.normalised(xy[:n], k0, k1)))
    pick = 0 if defect == "no vote" else int(v.argmax())
    R, tt = (R1, R2)[pick >> 1].copy(), (-1.0 if pick & 1 else 1.0) * t
    rows = xy[:n].astype(np.float64)
    done, status, steps = 0, 0, []
    for it in range(iters):
        sums = mr.pass_sums(rows, k0, k1, R, tt, scale_px)
        A, g, H = mr.damped(sums, tt)
        x = mr.solve6(A, g)
        new = mr.apply_step(R, tt, x) if x is not None else None
        if new is None:
            status = 1
            break
        steps.append({"A": A, "g": g, "H": H, "delta": x, "sums": sums, "R": R, "t": tt, "rows": rows, "cams": (k0, k1)})
        R, tt = new
        done += 1
    E, fin = unit_essential(mr.essential(R, tt).reshape(9))
    info = {"votes": v, "pick": pick, "done": done, "status": status if fin else 3, "R": R, "t": tt, "sigma": sigma, "small_depth": small,
            "steps": steps, "scale_px": scale_px}
    return (E if fin else np.zeros(9)), fin, info


def polish_bound(info):
    """What an entry of a polished E may differ by between two float64 evaluations of the rule: the split's bound
    (rr.split_bound) on the start, and per step the bound tests/test_gpu_matches.py holds cpn_refine_pose to
    (mr.refine_step_bound: its rotation and its translation entry, |t| = 1).  An entry of E = [t]x R is a difference of two
    products of an entry of t and one of R, all below 1: it moves by at most twice the sum of the two; the norm and the sign
    double it once more."""
    b = rr.split_bound(info["sigma"])
    for step in info["steps"]:
        _, b_rot, b_tr, _ = mr.refine_step_bound(step, info["scale_px"], 1.0)
        b += b_rot + b_tr
    return 4.0 * b


def polish_slots(Em, valid, partial, xy, count, intrinsics, K, inlier_px, iters, scale_px, defect=None):
    """The rule of cpn_ransac_polish for one pair: partial (chunks, >= Hn) holds the hypotheses' scores in its first Hn columns
    -> (E_lo (K, 9), valid_lo (K) uint8, info (K, 8) float64, ranks (K) the slots polished, details (K) polish's info or None)."""
    xy = np.asarray(xy, dtype=np.float32)
    Hn = len(Em)
    n = min(max(int(count), 0), len(xy))
    usable = int(np.isfinite(xy[:n]).all(axis=1).sum())
    used = -(-n // CHUNK)
    sums = np.asarray(partial)[:used, :Hn].sum(axis=0, dtype=np.int64)
    ranks = rank_list(sums, valid, K, usable, defect)
    E_lo, valid_lo, info, details = np.zeros((K, 9)), np.zeros(K, dtype=np.uint8), np.zeros((K, 8)), []
    for k, slot in enumerate(ranks):
        details.append(None)
        if slot < 0:
            info[k] = (-1, -1, 0, 0, 0, 0, 0, 2)
            continue
        E, fin, i = polish(Em[slot], xy, count, intrinsics, inlier_px, iters, scale_px, defect)
        E_lo[k], valid_lo[k], details[k] = E, 1 if fin else 0, i
        if i["status"] == 3 and "pick" not in i:                    # the split was not finite
            info[k] = (-1, -1, 0, 0, 0, 0, 0, 3)
        else:
            info[k] = (slot, k, i["done"], *i["votes"], i["status"])
    return E_lo, valid_lo, info, ranks, details


# ------------------------------------------------------------------------------------------------------------ the finish
def finish_lo(Em, valid, E_lo, valid_lo, info, partial, xy, count, intrinsics, inlier_px, graded, rel_pose=None, defect=None):
    """The rule of cpn_ransac_finish_lo for one pair: rr.finish over the Hn + K slots - its winner is the largest int64 sum,
    the lower slot on ties -, with the counts of the winner and of rel_pose taken from the matches where the score is graded
    -> (pose, inlier, stats, score, lo (4), info).  defect="last on ties"."""
    Hn, K = len(Em), len(E_lo)
    E_all = np.concatenate((np.asarray(Em, dtype=np.float64).reshape(Hn, 9), np.asarray(E_lo, dtype=np.float64).reshape(K, 9)))
    v_all = np.concatenate((np.asarray(valid).reshape(Hn), np.asarray(valid_lo).reshape(K))).astype(np.uint8)
    pose, inlier, stats, out = rr.finish(E_all, v_all, partial, xy, count, intrinsics, inlier_px, rel_pose, defect=defect)
    lo = np.array([0.0, -1.0, -1.0, 0.0])
    won = 0
    if stats[7] == 0:
        winner = int(stats[2])
        won = int(out["sums"][winner])
        if graded:
            stats[0] = float(inlier.sum())
        if winner >= Hn:
            lo = np.array([1.0, info[winner - Hn][0], info[winner - Hn][1], info[winner - Hn][2]])
    if graded and rel_pose is not None and stats[7] != 2:
        xy = np.asarray(xy, dtype=np.float32)
        n = min(max(int(count), 0), len(xy))
        stats[4] = float(rr.inliers(rr.rel_essential(rel_pose)[None], xy[:n], intrinsics, inlier_px)[0].sum())
    return pose, inlier, stats, won, lo, out


# ---------------------------------------------------------------------------------------------------------- the whole call
def hypotheses(xy, count, intrinsics, hypotheses_n, seed, solver="8pt"):
    """-> (E (slots, 9), valid (slots) uint8) of either solver: 10 slots per sample for "5pt"."""
    if solver == "5pt":
        Em, _, valid, _ = r5.hypotheses5(xy, count, intrinsics, hypotheses_n, seed)
        return Em.reshape(-1, 9), valid.reshape(-1)
    Em, _, valid = rr.hypotheses(xy, count, intrinsics, hypotheses_n, seed)
    return Em, valid


def ransac_pose(xy, count, intrinsics, rel_pose=None, hypotheses_n=1024, inlier_px=1.0, seed=0, solver="8pt", score_kind="inliers",
                lo=0, lo_iters=4, lo_scale_px=None, defect=None, hyp=None):
    """coponerf_amd.matches.ransac_pose's launches in a row for one pair -> dict: pose, inlier, stats, score, lo, and E, valid,
    E_lo, valid_lo, info, ranks, partial (chunks, slots + lo + 1) int32, sums.  hyp: (E, valid) already made."""
    graded = score_kind == "msac"
    Em, valid = hyp if hyp is not None else hypotheses(xy, count, intrinsics, hypotheses_n, seed, solver)
    Hn = len(Em)
    first = score(Em, valid, xy, count, intrinsics, inlier_px, graded, rel_pose, defect)
    partial = np.zeros((len(first), Hn + lo + 1), dtype=np.int32)
    partial[:, :Hn], partial[:, -1] = first[:, :Hn], first[:, Hn]
    E_lo, valid_lo, info, ranks, details = np.zeros((0, 9)), np.zeros(0, dtype=np.uint8), np.zeros((0, 8)), [], []
    if lo:
        scale = inlier_px if lo_scale_px is None else lo_scale_px
        E_lo, valid_lo, info, ranks, details = polish_slots(Em, valid, partial, xy, count, intrinsics, lo, inlier_px, lo_iters, scale, defect)
        partial[:, Hn:Hn + lo] = score(E_lo, valid_lo, xy, count, intrinsics, inlier_px, graded, None, defect)[:, :lo]
    pose, inlier, stats, won, lo_out, out = finish_lo(Em, valid, E_lo, valid_lo, info, partial, xy, count, intrinsics, inlier_px, graded,
                                                      rel_pose, defect)
    return {"pose": pose, "inlier": inlier, "stats": stats, "score": won, "lo": lo_out, "E": Em, "valid": valid, "E_lo": E_lo,
            "valid_lo": valid_lo, "info": info, "ranks": ranks, "details": details, "partial": partial, "sums": out["sums"], "finish": out}


# ------------------------------------------------------------------------------------------------------------- the scenes
SCENES = ("curved", "wall", "wall5")
SETTINGS = (("inliers", 0), ("msac", 0), ("inliers", 8), ("msac", 8))


@functools.lru_cache(maxsize=None)
def scene(name):
    """The three scenes of the accuracy table: tests/ransac_ref.py's noisy curved scene, tests/ransac5_ref.py's wall, and the
    wall with 5 % of its points off the plane.  1000 matches, 0.5 px noise, 30 % outliers."""
    if name == "curved":
        return mr.refine_scene(**rr.NOISY)
    return r5.wall_scene(**dict(r5.WALL, off_plane=0.05 if name == "wall5" else 0.0))


def accuracy_rows(sizes=(16, 64, 256, 1024), seeds=(0, 1, 2)):
    """The table of profiles/r24_lo_msac.json: per scene, solver, hypotheses, seed and setting the pose errors to the truth in
    degrees, of ransac_pose's pose and of cpn_refine_pose's restatement (10 passes, 2 px) from it, the winner's inliers, score
    and whether a polished slot won.  tools/lo_msac_time.py --accuracy writes it; tests/test_lo_msac_ref.py checks the rows it can
    afford to recompute."""
    rows = []
    for name in SCENES:
        sc = scene(name)
        for solver in ("8pt", "5pt"):
            for Hn in sizes:
                for seed in seeds:
                    hyp = hypotheses(sc["xy"], 1000, sc["intrinsics"], Hn, seed, solver)
                    for kind, lo in SETTINGS:
                        o = ransac_pose(sc["xy"], 1000, sc["intrinsics"], None, Hn, 1.0, seed, solver, kind, lo, hyp=hyp)
                        refined = mr.refine_pose(sc["xy"], 1000, sc["intrinsics"], o["pose"].astype(np.float32), 10, 2.0)[0]
                        rows.append({"scene": name, "solver": solver, "hypotheses": Hn, "seed": seed, "score": kind, "lo": lo,
                                     "status": int(o["stats"][7]), "inliers": int(o["stats"][0]), "winning_score": int(o["score"]),
                                     "polished_won": int(o["lo"][0]), "deg_R": mr.pose_errors(o["pose"], sc)[0],
                                     "deg_t": mr.pose_errors(o["pose"], sc)[1], "refined_deg_R": mr.pose_errors(refined, sc)[0],
                                     "refined_deg_t": mr.pose_errors(refined, sc)[1]})
    return rows



N_GPU, COUNTS_GPU = 768, (257, 511)
SEED_GPU = 2            # of seeds 0 .. 5 the first at which every fixture's winner leads by more than winner_margin's bound (0 and 1 do not)


@functools.lru_cache(maxsize=None)
def gpu_case():
    """The batch of tests/test_gpu_lo_msac.py: B = 2 pairs of N = 768 rows of the noisy curved scene, rows 0 .. and rows 232 ..,
    counts 257 (a chunk and one row) and 511 (one row short of two chunks), the third chunk all zeros; rel_pose the stalled
    start.  The walls are left to the accuracy table: their Gauss-Newton systems are so badly conditioned that the a-priori
    bound on a polished E (polish_bound) says nothing there, and the condition on the winner's margin cannot be shown.
    -> (xy (2, 768, 4) fp32, counts (2) int32, intrinsics (2, 2, 4, 4), rel_pose (2, 4, 4)).  Shared, never written to."""
    a = scene("curved")
    xy = np.stack((a["xy"][:N_GPU], a["xy"][232:232 + N_GPU])).copy()
    K = np.stack((a["intrinsics"], a["intrinsics"]))
    P = np.stack((rr.stalled_start(a), rr.stalled_start(a)))
    return xy, np.asarray(COUNTS_GPU, dtype=np.int32), K, P


@functools.lru_cache(maxsize=None)
def gpu_want(solver, hypotheses_n, score_kind, lo, with_rel=True, inlier_px=1.0, lo_iters=4, short=False):
    """The restatement's ransac_pose of every pair of gpu_case() (short: pair 0 cut to 7 matches, status 2; inlier_px == 0:
    lo_scale_px = 1, as the weights of the passes need a scale) -> list of dicts.  Shared, never written to."""
    xy, counts, K, P = gpu_case()
    counts = (7, counts[1]) if short else counts
    return [ransac_pose(xy[b], counts[b], K[b], P[b] if with_rel else None, hypotheses_n, inlier_px, SEED_GPU, solver, score_kind, lo, lo_iters,
                        None if inlier_px > 0.0 else 1.0) for b in range(2)]


def polished_score_bound(dE, e, xy, count, intrinsics, inlier_px, graded):
    """What the score of slot e (9) may differ by between two evaluations whose E differ by at most dE per entry.  To first
    order the residual r = n / sqrt(D) of a match moves by dr = (dn + |r| |d sqrt(D)|) / sqrt(D) with dn <= dE ca cb
    (ca = |a0| + |a1| + 1, cb likewise: n is a^T E b) and |d sqrt(D)| <= |dg| <= dE sqrt(cb^2 / fx0^2 + cb^2 / fy0^2 + ca^2 / fx1^2 +
    ca^2 / fy1^2) (D is |g|^2); twice that is taken.  A match with |r| within dr of the threshold may change sides - 1 for a
    count; for the graded score its weight there is below 2 ONE dr / px + 1, bounded by ONE -, and every other inlier's weight
    moves by at most 2 ONE |r| dr / px^2 + 1 (the floor)."""
    xy = np.asarray(xy, dtype=np.float32)
    n = min(max(int(count), 0), len(xy))
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    x = xy[:n].astype(np.float64)
    with np.errstate(all="ignore"):
        s = mr.sampson(np.asarray(e).reshape(3, 3), k0, k1, x[:, 0], x[:, 1], x[:, 2], x[:, 3])
        r, ok = mr.residual(s)
        ca, cb = np.abs(s["a0"]) + np.abs(s["a1"]) + 1.0, np.abs(s["b0"]) + np.abs(s["b1"]) + 1.0
        dg = dE * np.sqrt(cb * cb / k0[0] ** 2 + cb * cb / k0[1] ** 2 + ca * ca / k1[0] ** 2 + ca * ca / k1[1] ** 2)
        dr = 2.0 * (dE * ca * cb + np.abs(r) * dg) / np.sqrt(s["D"])
        near = ok & (np.abs(np.abs(r) - inlier_px) <= dr)
        inl = ok & (np.abs(r) <= inlier_px) & ~near
    if not graded:
        return int(near.sum())
    move = 2.0 * ONE * np.abs(r[inl]) * dr[inl] / (inlier_px * inlier_px) + 1.0
    return int(near.sum()) * ONE + int(np.ceil(move.sum()))


def winner_margin(out, xy, count, intrinsics, inlier_px, graded):
    """Of ransac_pose's dict: (the winner, the runner-up, the winner's score minus the runner-up's, what the scores of those of
    the two that are polished slots may move by when their E moves by polish_bound - 0: both scores are exact)."""
    Hn, lo = len(out["E"]), len(out["E_lo"])
    valid = np.concatenate((out["valid"], out["valid_lo"]))
    sums = out["sums"][:Hn + lo]
    order = [int(h) for h in np.lexsort((np.arange(Hn + lo), -sums)) if valid[h]]
    first, second = order[0], order[1]
    bound = 0
    for h in (first, second):
        if h >= Hn and inlier_px > 0.0:
            bound += polished_score_bound(polish_bound(out["details"][h - Hn]), out["E_lo"][h - Hn], xy, count, intrinsics, inlier_px, graded)
    return first, second, int(sums[first] - sums[second]), bound
