"""CPU: the restatement of pruned scan matching (tests/scan_match_pruned_restatement.py) against the exhaustive restatement
(tests/scan_match_restatement.py) -- the same seven result members on every shared case -- and against its own contract: the bound
planes are block maxima, a bound is no smaller than any score under it nor than its children's bounds, the counters add up, and
the search prunes (a search that evaluates everything gives the same answer and must not pass)."""
import math

import numpy as np
import pytest

import gridmap_cases as gc
import scan_match_cases as smc
import scan_match_pruned_cases as pc
import scan_match_pruned_restatement as sp
import scan_match_restatement as sm

F = np.float32
DEG = math.radians(1.0)


def _same(got, want, what=""):
    assert got["robot_in_world"].tobytes() == want["robot_in_world"].tobytes(), "pose " + what
    for k in pc.MEMBERS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), "%s %s: %s != %s" % (k, what, got[k], want[k])


def test_bound_planes_are_block_maxima():
    field = np.random.default_rng(1).integers(0, 256, (11, 7)).astype(np.uint8)
    field[field < 200] = 0
    planes = sp.bound_planes(field, 4)
    for l, P in enumerate(planes):
        s = 1 << l
        assert P.shape == (11 + s - 1, 7 + s - 1) and P.dtype == np.uint8
        for y in range(-(s - 1), 11):
            for x in range(-(s - 1), 7):
                block = field[max(y, 0):min(y + s, 11), max(x, 0):min(x + s, 7)]
                assert P[y + s - 1, x + s - 1] == block.max(initial=0), (l, x, y)
    empty = sp.bound_planes(np.zeros((0, 9), np.uint8), 2)
    assert empty[1].shape == (1, 10) and empty[2].shape == (3, 12) and not empty[2].any()


@pytest.mark.parametrize("window", ((3, 4, 1), (7, 8, 1), (8, 1, 2), (0, 0, 0), (1, 0, 1)), ids=str)
def test_bounds_hold_and_counters_add_up(window):
    """against a brute-force block maximum of the exhaustive volume: U_l >= every score of the block, U_(l+1) of the parent >= U_l
    of the child; every evaluated child has a surviving parent; num_evaluated[l - 1] <= 4 num_survivors[l]"""
    rm = smc.recovery_map()
    g, sc, field = rm["g"], rm["sc"], rm["field"]
    truth, scans, guesses = pc.recovery_batch()
    wx, wy, ht = window
    nx, ny = 2 * wx + 1, 2 * wy + 1
    planes = pc.recovery_planes()
    for k in (0, 3):
        guess = (truth[k] @ gc.pose(0.11, -0.07, 0.02)).astype(F)
        vol = sm.volume(field, scans[k:k + 1], guess[None], sc, g, wx, wy, ht, 0.02)[0][0]
        cells = sp.live_cells(scans[k], guess, sc, g, wx, wy, ht, 0.02)
        for levels in (1, 2, 3, 4):
            trace = {}
            flat, score, at_guess, st = sp.search(field, planes, cells, wx, wy, ht, levels, trace=trace)
            assert flat == sm.best(vol, wx, wy, ht) and score == vol.reshape(-1)[flat] and at_guess == vol[ht, wy, wx]
            assert st["floor_score"] <= score and st["num_evaluated"][levels] == len(trace[levels]["U"])
            for l in range(levels, 0, -1):
                s, t = 1 << l, trace[l]
                for j, by, bx, U in zip(t["jj"], t["by"], t["bx"], t["U"]):
                    assert U >= vol[j, by * s:by * s + s, bx * s:bx * s + s].max(), (l, j, by, bx)
                assert st["num_survivors"][l] == t["alive"].sum() and st["num_evaluated"][l - 1] <= 4 * st["num_survivors"][l]
                # the children evaluated below are exactly the children inside the window of this level's survivors
                parents = {(j, by, bx): U for j, by, bx, U, a in zip(t["jj"], t["by"], t["bx"], t["U"], t["alive"]) if a}
                kids = trace[l - 1]
                assert len(kids["U"]) == st["num_evaluated"][l - 1]
                for j, by, bx, U in zip(kids["jj"], kids["by"], kids["bx"], kids["U"]):
                    assert (j, by // 2, bx // 2) in parents and parents[(j, by // 2, bx // 2)] >= U
            # level 0 holds scores
            for j, y, x, U in zip(trace[0]["jj"], trace[0]["by"], trace[0]["bx"], trace[0]["U"]):
                assert U == vol[j, y, x]


def test_the_exhaustive_answer_on_the_shared_cases():
    """recovery trials, windows with hanging blocks, guesses outside the grid, scans without returns, an empty field"""
    rm = smc.recovery_map()
    g, sc, field = rm["g"], rm["sc"], rm["field"]
    truth, scans, guesses = pc.recovery_batch()
    planes = pc.recovery_planes()
    batch = np.concatenate([scans[:3], np.full((1, 361), np.nan, F), np.full((1, 361), 25.0, F)])
    gs = np.concatenate([guesses[:3], guesses[3:4], np.stack([gc.pose(-3.0, -2.0, 1.0)]).astype(F)])
    for window, step in (((12, 12, 10), DEG), ((4, 7, 0), 0.0), ((1, 0, 1), 0.3)):
        want = sm.match(field, batch, gs, sc, g, *window, step)
        for levels in (1, 2, 3, 4, 6):
            _same(sp.match(field, batch, gs, sc, g, *window, step, levels, planes=planes), want, "%s %d" % (window, levels))
        for limit in (1, 4):
            got = sp.match(field, batch, gs, sc, g, *window, step, 3, limit, planes=planes)
            _same(got, want, "limit %d" % limit)
            for st in got["stats"]:
                assert st["fell_back"] == (st["num_evaluated"][0] == st["num_candidates"]) or st["num_candidates"] <= limit
    zero = np.zeros_like(field)
    got = sp.match(zero, batch, gs, sc, g, 5, 5, 2, DEG, 3)
    _same(got, sm.match(zero, batch, gs, sc, g, 5, 5, 2, DEG))
    assert all(st["num_survivors"] == [0] * 7 and st["floor_score"] == 0 for st in got["stats"]) and not got["dx"].any()


def test_a_fall_back_keeps_the_levels_above_the_overflow():
    rm = smc.recovery_map()
    truth, scans, guesses = pc.recovery_batch()
    free = sp.match(rm["field"], scans[:1], guesses[:1], rm["sc"], rm["g"], 12, 12, 10, DEG, 4, planes=pc.recovery_planes())["stats"][0]
    assert free["fell_back"] == 0 and min(free["num_evaluated"][:5]) > 0
    limit = max(free["num_evaluated"][2:4])  # lets levels 3 and 2 through; level 1 or 0 holds more
    assert max(free["num_evaluated"][:2]) > limit
    over = 1 if free["num_evaluated"][1] > limit else 0
    st = sp.match(rm["field"], scans[:1], guesses[:1], rm["sc"], rm["g"], 12, 12, 10, DEG, 4, limit, planes=pc.recovery_planes())["stats"][0]
    assert st["fell_back"] == 1 and st["num_evaluated"][0] == st["num_candidates"] == 25 * 25 * 21
    assert st["num_evaluated"][over + 1:] == free["num_evaluated"][over + 1:] and st["num_survivors"][over + 1:] == free["num_survivors"][over + 1:]
    assert st["num_evaluated"][1:over + 1] == [0] * over and st["num_survivors"][:over + 1] == [0] * (over + 1)
    assert (st["floor_score"], st["seed_block"]) == (free["floor_score"], free["seed_block"])


def test_it_prunes():
    """recovery trials 0 .. 9, the 81 x 81 x 41 window at 1 degree: the score evaluations of a search -- top-level bounds, seed
    block, guess and everything below -- are at most a third of the candidates at one level and an eighth at two, three and four"""
    rm = smc.recovery_map()
    truth, scans, guesses = pc.recovery_batch()
    planes = pc.recovery_planes()
    for k in range(10):
        cells = sp.live_cells(scans[k], guesses[k], rm["sc"], rm["g"], 40, 40, 20, DEG)
        for levels, share in ((1, 3), (2, 8), (3, 8), (4, 8)):
            st = sp.search(rm["field"], planes, cells, 40, 40, 20, levels)[3]
            count = sp.evaluations(st, levels)
            print("trial %d, %d levels: %d candidates / %d evaluations = %.1f" % (k, levels, st["num_candidates"], count, st["num_candidates"] / count))
            assert st["num_candidates"] == 81 * 81 * 41 and count * share <= st["num_candidates"], (k, levels)
