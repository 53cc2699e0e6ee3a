"""tests/lo_msac_ref.py, the numpy restatement of round 24's LO-MSAC (cpn_ransac_score_slots, cpn_ransac_polish,
cpn_ransac_finish_lo) that tests/test_gpu_lo_msac.py compares the kernels with, pinned on the CPU: the graded score against a
brute-force sum of Python integers, the fixtures' decision margins, the rank against np.lexsort, the winning-score property, the
polish without passes against the split's own algebra, four seeded defects, and the accuracy table of profiles/r24_lo_msac.json.
"""
import json
import math
import os

import numpy as np
import pytest

from tests import lo_msac_ref as lm
from tests import matches_ref as mr
from tests import ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "r24_lo_msac.json")

# every configuration tests/test_gpu_lo_msac.py runs: (solver, hypotheses, score, lo, rel_pose given, inlier_px, lo_iters, short)
GPU_CONFIGS = [("8pt", 40, "msac", 8, True, 1.0, 4, False), ("8pt", 40, "inliers", 8, True, 1.0, 4, False),
               ("8pt", 40, "msac", 1, False, 1.0, 4, False), ("8pt", 4, "msac", 8, True, 1.0, 4, False),
               ("8pt", 40, "msac", 0, True, 1.0, 4, False), ("8pt", 40, "msac", 8, True, 0.0, 4, False),
               ("8pt", 40, "msac", 8, True, 1.0, 4, True), ("5pt", 30, "msac", 8, True, 1.0, 4, False),
               ("5pt", 30, "inliers", 1, False, 1.0, 4, False)]


def _all_slots(out):
    return np.concatenate((out["E"], out["E_lo"].reshape(-1, 9))), np.concatenate((out["valid"], out["valid_lo"]))


# ------------------------------------------------------------------------------------------------------------- the score
@pytest.mark.parametrize("px", (1.0, 0.37, 0.0))
def test_msac_score_is_the_brute_force_sum(px):
    """Every slot of the GPU fixture (40 eight-point hypotheses and rel_pose's slot, both pairs): the restatement's partials,
    summed, equal a loop over the matches in Python integers straight from the definition - 0 for no inlier,
    floor(2^20 (1 - r^2 / px^2)) held to [0, 2^20], 2^20 for px == 0 - and no chunk exceeds 2^28."""
    xy, counts, K, P = lm.gpu_case()
    for b in range(2):
        Em, valid = lm.hypotheses(xy[b], counts[b], K[b], 40, 0)
        part = lm.score(Em, valid, xy[b], counts[b], K[b], px, True, P[b])
        assert part.dtype == np.int32 and part.shape == (3, 41) and not part[2].any() and part.max() <= 2 ** 28
        slots = np.concatenate((Em, rr.rel_essential(P[b])[None]))
        r, ok = rr.residuals(slots, xy[b][:counts[b]], K[b])
        for h in range(41):
            total = 0
            if h == 40 or valid[h]:
                for i in range(counts[b]):
                    if ok[h, i] and abs(r[h, i]) <= px:
                        w = (1 << 20) if px == 0.0 else math.floor(2 ** 20 * (1.0 - r[h, i] * r[h, i] / (px * px)))
                        total += min(max(w, 0), 1 << 20)
            assert total == int(part[:, h].astype(np.int64).sum()), (b, h)
        counts_part = lm.score(Em, valid, xy[b], counts[b], K[b], px, False, P[b])
        assert np.array_equal(counts_part, rr.score(Em, valid, xy[b], counts[b], K[b], px, P[b]))       # round 20's counts
        assert (part.astype(np.int64) <= counts_part.astype(np.int64) << 20).all()


def test_scores_beyond_int32_are_summed_in_int64():
    """2^12 chunks of 2^28 reach 2^40: the finish sums in int64 and compares (score, slot) pairs."""
    part = np.full((4096, 3), 2 ** 28, dtype=np.int32)
    part[0, 1] += 1
    sums = part.sum(axis=0, dtype=np.int64)
    assert sums[1] == 2 ** 40 + 1 and lm.ranked_slot(sums, [True] * 3, 0) == (2 ** 40 + 1, 1)
    assert lm.rank_list(sums, [1, 1, 1], 4) == [1, 0, 2, -1]


@pytest.mark.parametrize("config", GPU_CONFIGS)
def test_fixture_decision_margins(config):
    """What lets tests/test_gpu_lo_msac.py compare decisions exactly.  For every slot the kernels score - the hypotheses, the
    polished slots, rel_pose's - no match lies within rr.MARGIN = 1e-9 px of the threshold and no weight's value before the
    floor within FLOOR_MARGIN = 1e-6 of an integer (two float64 evaluations differ by about 2e-9 there).  And the winner's
    margin over the runner-up exceeds what the scores of the polished slots may move by when their E moves by polish_bound,
    the bound cpn_refine_pose is held to: where neither is a polished slot, or no match can change sides under a count, the
    scores are exact and there is nothing to show.  inlier_px == 0 has no margin to keep: its inliers are the residuals that ARE
    zero - the slot's own sample -, decided by one IEEE sequence of + - * / sqrt on either side."""
    solver, Hn, kind, lo, with_rel, px, iters, short = config
    xy, counts, K, P = lm.gpu_case()
    for b, out in enumerate(lm.gpu_want(*config)):
        n = 7 if (short and b == 0) else counts[b]
        Em, valid = _all_slots(out)
        if with_rel:
            Em, valid = np.concatenate((Em, rr.rel_essential(P[b])[None])), np.concatenate((valid, [1]))
        r, ok = lm.residual_table(Em, valid, xy[b][:n], K[b])
        gap = np.abs(np.abs(r) - px)[ok]
        _, _, v = lm.weights(r, ok, px)
        print(config, "pair", b, "threshold margin", gap.min() if len(gap) else np.inf, "floor margin", lm.floor_margin(v, r, px),
              "status", out["stats"][7], "winner", out["stats"][2], "lo", out["lo"])
        assert len(gap) == 0 or gap.min() >= rr.MARGIN or px == 0.0
        assert lm.floor_margin(v, r, px) >= lm.FLOOR_MARGIN
        if out["stats"][7] != 0 or lo == 0:
            continue
        first, second, margin, bound = lm.winner_margin(out, xy[b], n, K[b], px, kind == "msac")
        assert first == out["stats"][2]
        print("    margin", margin, "bound", bound)
        assert bound == 0 or margin > bound


# -------------------------------------------------------------------------------------------------------------- the rank
def test_rank_is_lexsort_and_stops_at_the_valid_slots():
    """rank_list - per rank the kernel's sweep: a sorted chain of 16 per thread, then the heads taken one by one - equals
    np.lexsort on (slot, -score) over the valid slots, with ties in the scores and with more slots than threads (several slots
    and ties inside one thread's chain); ranks beyond the valid slots, and every rank with fewer than 8 usable matches, are -1."""
    rng = np.random.default_rng(24)
    for trial in range(20):
        H = int(rng.integers(1, 40)) if trial % 2 else int(rng.integers(600, 6000))
        sums = rng.integers(0, 6, size=H).astype(np.int64) * (1 << 33)         # many ties, beyond 32 bits
        valid = (rng.random(H) < 0.7).astype(np.uint8)
        want = [int(h) for h in np.lexsort((np.arange(H), -sums)) if valid[h]]
        got = lm.rank_list(sums, valid, 16)
        assert got == (want + [-1] * 16)[:16], trial
        assert lm.rank_list(sums, valid, 4, usable=7) == [-1] * 4
    out = lm.gpu_want("8pt", 4, "msac", 8)                          # 4 hypotheses, K = 8: ranks 4 .. 7 have nothing to polish
    for o in out:
        nv = int(o["valid"].sum())
        assert nv <= 4 and all(s >= 0 for s in o["ranks"][:nv]) and o["ranks"][nv:] == [-1] * (8 - nv)
        assert not o["valid_lo"][nv:].any() and not o["E_lo"][nv:].any()
        assert (o["info"][nv:] == np.array([-1, -1, 0, 0, 0, 0, 0, 2.0])).all() and o["stats"][3] == nv + o["valid_lo"].sum()
    short = lm.gpu_want("8pt", 40, "msac", 8, short=True)[0]       # 7 matches: status 2, nothing polished
    assert short["stats"][7] == 2 and short["ranks"] == [-1] * 8 and short["score"] == 0 and not short["valid_lo"].any()


# -------------------------------------------------------------------------------------------------------------- property
@pytest.mark.parametrize("config", GPU_CONFIGS)
def test_winning_score_never_falls_with_lo(config):
    """A polished slot carries a higher index than every hypothesis and ties go to the lower index: with lo = K the winning
    score is at least the score with lo = 0, on every fixture pair, under either score."""
    solver, Hn, kind, lo, with_rel, px, iters, short = config
    with_lo = lm.gpu_want(*config)
    without = lm.gpu_want(solver, Hn, kind, 0, with_rel, px, iters, short)
    for a, b in zip(with_lo, without):
        assert a["stats"][7] == b["stats"][7] and a["score"] >= b["score"]
        assert np.array_equal(a["partial"][:, :len(b["E"])], b["partial"][:, :-1])            # the hypotheses score alike
        if a["lo"][0]:
            assert a["score"] > b["score"] and a["stats"][2] >= len(a["E"])


def test_a_polished_slot_that_ties_does_not_win():
    """The winner's own E as the polished slot: the same score, the higher slot - the hypothesis keeps the win, lo says so."""
    xy, counts, K, P = lm.gpu_case()
    for kind in ("inliers", "msac"):
        base = lm.gpu_want("8pt", 40, kind, 0)[0]
        w = int(base["stats"][2])
        E_lo, valid_lo = base["E"][w][None], np.ones(1, dtype=np.uint8)
        info = np.array([[w, 0, 0, 0, 0, 0, 0, 0.0]])
        graded = kind == "msac"
        partial = np.zeros((3, 42), dtype=np.int32)
        partial[:, :40], partial[:, 41] = base["partial"][:, :40], base["partial"][:, 40]
        partial[:, 40] = lm.score(E_lo, valid_lo, xy[0], counts[0], K[0], 1.0, graded)[:, 0]
        assert np.array_equal(partial[:, 40], partial[:, w])
        pose, inlier, stats, won, lo, _ = lm.finish_lo(base["E"], base["valid"], E_lo, valid_lo, info, partial, xy[0], counts[0], K[0],
                                                       1.0, graded, P[0])
        assert stats[2] == w and won == base["score"] and lo[0] == 0 and np.array_equal(pose, base["pose"])
        assert np.array_equal(stats, base["stats"] + np.array([0, 0, 0, 1.0, 0, 0, 0, 0]))     # one more valid slot, nothing else


# ---------------------------------------------------------------------------------------------------------- lo_iters = 0
@pytest.mark.parametrize("solver,Hn", (("8pt", 40), ("5pt", 30)))
def test_no_passes_reproduce_the_source_slot_up_to_the_split(solver, Hn):
    """lo_iters = 0 writes [t]x R of the split as it is.  With sigma the column norms of the split of the unit-norm source E
    = U diag(sigma) V^T, [t]x R normalised is +-U diag(1, 1, 0) V^T / sqrt(2), so |E_lo -+ E|_F IS
    sqrt((sigma_1 - 1 / sqrt(2))^2 + (sigma_2 - 1 / sqrt(2))^2 + sigma_3^2) up to the split's rounding: the bound stated and
    held is that distance + 36 rr.split_bound(sigma) + 1e-12 (9 entries, 4 split bounds each, as lm.polish_bound counts them) -
    and the distance itself is met to the same slack.  A 5-point slot is an essential matrix already: its distance is below
    1e-9; an 8-point slot is not, and the polish without passes is its projection."""
    for o in lm.gpu_want(solver, Hn, "msac", 8, True, 1.0, 0):
        assert o["stats"][7] == 0 and o["valid_lo"].all() and (o["info"][:, 2] == 0).all() and (o["info"][:, 7] == 0).all()
        worst = 0.0
        for k, slot in enumerate(o["ranks"]):
            e, sigma = o["E"][slot], o["details"][k]["sigma"]
            dist = math.sqrt((sigma[0] - math.sqrt(0.5)) ** 2 + (sigma[1] - math.sqrt(0.5)) ** 2 + sigma[2] ** 2)
            slack = 36.0 * rr.split_bound(sigma) + 1e-12
            got = min(np.linalg.norm(o["E_lo"][k] - e), np.linalg.norm(o["E_lo"][k] + e))
            assert got <= dist + slack and abs(got - dist) <= slack, (k, got, dist, slack)
            worst = max(worst, dist)
        print(solver, "largest distance of a source slot from its projection", worst)
        assert worst < 1e-9 or solver == "8pt"


# -------------------------------------------------------------------------------------------------------- seeded defects
def test_seeded_defects_are_caught():
    """Round in place of floor: the brute-force sum differs.  Ties to the higher index: the tie fixture's winner and rank
    change.  A rank that skips a slot: the rank list is not lexsort's.  The vote left out of the polish: the polished slots'
    info - the votes, and with them the candidate the passes start from - differs, and the tie fixture (every candidate but
    the voted one puts its points behind a camera) shows a start that is not the voted pose."""
    xy, counts, K, P = lm.gpu_case()
    Em, valid = lm.hypotheses(xy[0], counts[0], K[0], 40, 0)
    good = lm.score(Em, valid, xy[0], counts[0], K[0], 1.0, True)
    bad = lm.score(Em, valid, xy[0], counts[0], K[0], 1.0, True, defect="round")
    assert not np.array_equal(good, bad) and (bad >= good).all()

    exact = mr.refine_scene(**rr.EXACT)
    tie = lm.ransac_pose(exact["xy"], 1000, exact["intrinsics"], None, 16, 1.0, 0, "8pt", "inliers", 4)
    late = lm.ransac_pose(exact["xy"], 1000, exact["intrinsics"], None, 16, 1.0, 0, "8pt", "inliers", 4, defect="last on ties")
    top = np.flatnonzero(tie["sums"][:16] == tie["sums"][:16].max())
    assert len(top) > 4 and tie["ranks"] == list(top[:4]) and tie["stats"][2] == top[0] and tie["lo"][0] == 0
    assert late["ranks"] != tie["ranks"] and late["stats"][2] != tie["stats"][2]

    sums, ok = tie["sums"][:16], tie["valid"]
    want = [int(h) for h in np.lexsort((np.arange(16), -sums)) if ok[h]][:8]
    assert lm.rank_list(sums, ok, 8) == want
    many = np.zeros(700, dtype=np.int64)                            # slots 5 and 261 are one thread's: its chain holds both
    many[[5, 261, 7]] = (10, 9, 8)
    assert lm.rank_list(many, np.ones(700), 4) == [5, 261, 7, 0]
    assert lm.rank_list(many, np.ones(700), 4, defect="skips a slot") == [5, 7, 0, 1]

    voted = lm.polish_slots(tie["E"], tie["valid"], tie["partial"], exact["xy"], 1000, exact["intrinsics"], 4, 1.0, 4, 1.0)
    blind = lm.polish_slots(tie["E"], tie["valid"], tie["partial"], exact["xy"], 1000, exact["intrinsics"], 4, 1.0, 4, 1.0, defect="no vote")
    picks = [d["pick"] for d in voted[4]]
    assert np.array_equal(voted[2], blind[2]) and any(picks)       # the info is the votes' either way; the start is not
    for a, b in zip(voted[4], blind[4]):
        assert a["votes"].max() == 1000 and (np.sort(a["votes"])[:3] == 0).all()             # exact matches: one candidate has them all
        if a["pick"]:
            assert mr.rotation_angle_deg(a["R"], exact["R_true"]) < 1e-6 and mr.direction_angle_deg(a["t"], exact["t_true"]) < 1e-6
            off = max(mr.rotation_angle_deg(b["R"], exact["R_true"]), mr.direction_angle_deg(b["t"], exact["t_true"]))
            assert off > 10.0                                       # the passes without the vote end at a twisted or mirrored pose


# ----------------------------------------------------------------------------------------------------- the accuracy table
def test_accuracy_table_rows():
    """Three scenes, both solvers, 16 and 64 hypotheses, seeds 0 - 2, the four settings: every result is finite with status 0,
    the winning score with lo = 8 is at least the score with lo = 0 under the same score, and the rows are the ones
    profiles/r24_lo_msac.json records (which holds 256 and 1024 hypotheses as well).  Nothing is asserted about the errors:
    the README reports them, the cells where LO-MSAC is no nearer the truth than round 20's loop included."""
    rows = lm.accuracy_rows(sizes=(16, 64))
    assert len(rows) == 3 * 2 * 2 * 3 * 4
    key = lambda r: (r["scene"], r["solver"], r["hypotheses"], r["seed"], r["score"], r["lo"])
    by = {key(r): r for r in rows}
    for r in rows:
        assert r["status"] == 0 and all(math.isfinite(r[k]) for k in ("deg_R", "deg_t", "refined_deg_R", "refined_deg_t")), r
        if r["lo"]:
            assert r["winning_score"] >= by[key(r)[:5] + (0,)]["winning_score"], r
    with open(TABLE) as f:
        recorded = {key(r): r for r in json.load(f)["accuracy"]["rows"]}
    assert len(recorded) == 3 * 2 * 4 * 3 * 4
    for k, r in by.items():
        got = recorded[k]
        assert all(got[f] == r[f] for f in ("status", "inliers", "winning_score", "polished_won")), (k, got, r)
        assert all(abs(got[f] - r[f]) <= 1e-9 for f in ("deg_R", "deg_t", "refined_deg_R", "refined_deg_t")), (k, got, r)
    for r in recorded.values():
        assert r["status"] == 0
        if r["lo"]:
            assert r["winning_score"] >= recorded[key(r)[:5] + (0,)]["winning_score"], r
