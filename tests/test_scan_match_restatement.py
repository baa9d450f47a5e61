"""CPU: the numpy restatement of correlative scan matching (tests/scan_match_restatement.py) against a per-candidate, per-beam
Python loop on tiny shapes, the properties of its contract, and the recovery setting: ten seeded trials up to 0.6 m per axis and
10 degrees off must each come back within one cell per axis and one angle step."""
import math

import numpy as np
import pytest

import gridmap_cases as gc
import gridmap_restatement as gr
import scan_match_cases as sc_
import scan_match_restatement as sm

F = np.float32


def _loop_field(occ, R, lut):
    rows, cols = occ.shape
    out = np.zeros((rows, cols), np.uint8)
    for y in range(rows):
        for x in range(cols):
            top = 0
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    if dx * dx + dy * dy <= R * R and 0 <= y + dy < rows and 0 <= x + dx < cols and occ[y + dy, x + dx]:
                        top = max(top, int(lut[dx * dx + dy * dy]))
            out[y, x] = top
    return out


def _loop_volume(field, ranges, guesses, sc, g, wx, wy, ht, step):
    K = guesses.shape[0]
    rows, cols = field.shape
    vol = np.zeros((K, 2 * ht + 1, 2 * wy + 1, 2 * wx + 1), np.int32)
    for j in range(-ht, ht + 1):
        ok, x1, y1 = sm.end_cells(ranges, guesses, sc, g, j, step, ht)
        for k in range(K):
            for dy in range(-wy, wy + 1):
                for dx in range(-wx, wx + 1):
                    s = 0
                    for b in range(sc["num_beams"]):
                        if ok[k, b] and 0 <= x1[k, b] + dx < cols and 0 <= y1[k, b] + dy < rows:
                            s += int(field[y1[k, b] + dy, x1[k, b] + dx])
                    vol[k, j + ht, dy + wy, dx + wx] = s
    return vol


def _tiny(rows, cols, K, nb, seed):
    g, sc, poses, ranges = gc.shape_case(((rows, cols), K, nb), seed=seed)
    h, w = gr.new_planes(g)
    gr.integrate(h, w, ranges, poses, sc, g)
    return g, sc, poses, gc.mixed(ranges, seed + 1), h, w


@pytest.mark.parametrize("rows,cols,R", ((1, 1, 0), (1, 9, 1), (7, 5, 4), (7, 5, 16), (20, 23, 4)))
def test_the_field_is_the_loop(rows, cols, R):
    rng = np.random.default_rng(rows * 100 + cols + R)
    occ = rng.random((rows, cols)) < 0.15
    occ[0, 0] = occ[-1, -1] = True
    lut = sm.default_lut(R)
    assert lut[0] == 255 and (R == 0 or lut[-1] < lut[0]) and np.all(np.diff(lut.astype(int)) <= 0)
    assert np.array_equal(sm.dilate(occ, R, lut), _loop_field(occ, R, lut))
    wild = rng.integers(0, 256, R * R + 1).astype(np.uint8)  # not monotone: the maximum decides, not the nearest cell
    assert np.array_equal(sm.dilate(occ, R, wild), _loop_field(occ, R, wild))


def test_a_non_monotone_table_takes_the_maximum_not_the_nearest():
    occ = np.zeros((5, 9), bool)
    occ[2, 2] = occ[2, 6] = True
    lut = np.zeros(17, np.uint8)
    lut[1], lut[9] = 10, 200  # a cell one away scores 10, three away 200
    f = sm.dilate(occ, 4, lut)
    assert f[2, 3] == 200  # (2, 6) is three away and beats the neighbour (2, 2)
    assert f[2, 1] == 10 and f[2, 2] == 0 and f[0, 0] == 0


def test_the_default_table_is_the_formula():
    for R in range(17):
        n = R * R + 1
        assert list(sm.default_lut(R)) == [(255 * (n - d)) // n for d in range(n)]


@pytest.mark.parametrize("shape,window", (((7, 5, 2, 16), (1, 1, 1)), ((20, 23, 2, 33), (3, 2, 2)), ((20, 23, 1, 16), (0, 0, 0)),
                                          ((1, 9, 1, 8), (9, 0, 0)), ((20, 23, 1, 16), (0, 25, 0))))
def test_the_volume_is_the_loop(shape, window):
    g, sc, poses, ranges, h, w = _tiny(*shape, seed=7)
    field = sm.likelihood(h, w, 1, 50, 2, sm.default_lut(2))
    assert field.any()
    wx, wy, ht = window
    guesses = np.stack([p @ gc.pose(0.07, -0.04, 0.05) for p in poses]).astype(F)
    got = sm.match(field, ranges, guesses, sc, g, wx, wy, ht, 0.03)
    want = _loop_volume(field, ranges, guesses, sc, g, wx, wy, ht, 0.03)
    assert np.array_equal(got["scores"], want)
    for k in range(shape[2]):
        flat = want[k].reshape(-1)
        win = ((got["jtheta"][k] + ht) * (2 * wy + 1) + got["dy"][k] + wy) * (2 * wx + 1) + got["dx"][k] + wx
        assert flat[win] == flat.max() == got["score"][k] and got["score_at_guess"][k] == want[k, ht, wy, wx]
    assert np.array_equal(got["num_scored_beams"], gr.classify(ranges, sc)[0].sum(axis=1))


def test_shifting_the_field_by_whole_cells_shifts_the_arg_max():
    g = gr.grid(40, 44, 0.05, (-1.0, 0.5))
    sc = gr.scanner(*gc.fan(65), 65, range_min=0.02, range_max=20.0)
    room = gc.room_of(g, margin=0.3)  # (a margin of empty cells to shift into)
    poses = gc.trajectory(room, 1, 11)
    ranges = gc.room_scans(room, poses, sc, sigma=0.004, seed=12)
    h, w = gr.new_planes(g)
    gr.integrate(h, w, ranges, poses, sc, g)
    field = sm.likelihood(h, w, 1, 50, 2, sm.default_lut(2))
    assert field.any() and not field[:6].any() and not field[-6:].any() and not field[:, :6].any() and not field[:, -6:].any()
    a = sm.match(field, ranges, poses, sc, g, 6, 6, 0, 0.0)
    assert a["score"][0] > 0 and abs(a["dx"][0]) <= 2 and abs(a["dy"][0]) <= 2
    for sx, sy in ((2, 0), (0, -3), (-1, 2)):
        b = sm.match(np.roll(field, (sy, sx), (0, 1)), ranges, poses, sc, g, 6, 6, 0, 0.0)
        assert (b["dx"][0], b["dy"][0], b["score"][0]) == (a["dx"][0] + sx, a["dy"][0] + sy, a["score"][0])
        assert np.array_equal(b["scores"][0, 0, 3:10, 3:10], a["scores"][0, 0, 3 - sy:10 - sy, 3 - sx:10 - sx])
        want = F(a["robot_in_world"][0, 0, 2] - F(a["dx"][0]) * g["res"]) + F(b["dx"][0]) * g["res"]
        assert b["robot_in_world"][0, 0, 2] == want


def test_an_empty_field_no_returns_and_an_empty_grid_hand_the_guess_back():
    g, sc, poses, ranges, h, w = _tiny(20, 23, 2, 16, seed=13)
    guesses = np.stack([p @ gc.pose(0.02, 0.01, 0.3) for p in poses]).astype(F)
    for field, r in ((np.zeros((20, 23), np.uint8), ranges), (np.full((20, 23), 9, np.uint8), np.full_like(ranges, np.nan))):
        out = sm.match(field, r, guesses, sc, g, 2, 3, 2, 0.1)
        assert not out["scores"].any() and not out["dx"].any() and not out["dy"].any() and not out["jtheta"].any()
        assert out["robot_in_world"].tobytes() == sm.rotated_guesses(guesses, 0, 0.1, 2).tobytes()
        assert np.array_equal(out["robot_in_world"][:, :2, :], guesses[:, :2, :])  # turning by nothing changes nothing
    out = sm.match(np.zeros((0, 9), np.uint8), ranges, guesses, sc, gr.grid(0, 9), 1, 1, 1, 0.1)
    assert not out["scores"].any() and out["scores"].shape == (2, 3, 3, 3) and out["num_scored_beams"].sum() > 0


def test_the_tie_order():
    vol = np.zeros((3, 3, 5), np.int32)  # ht = 1, wy = 1, wx = 2: the guess is flat index 22
    assert sm.best(vol, 2, 1, 1) == 22
    vol[0, 2, 4] = vol[2, 0, 1] = 7
    assert sm.best(vol, 2, 1, 1) == 14  # two equal maxima: the lowest flat index
    vol[1, 1, 2] = 7
    assert sm.best(vol, 2, 1, 1) == 22  # the guess among the maxima
    vol[2, 2, 4] = 8
    assert sm.best(vol, 2, 1, 1) == 44


def test_recovery_ten_seeded_trials_within_one_cell_and_one_step():
    """the setting quoted in DESIGN.md: window +-14 cells and +-12 steps of one degree"""
    m = sc_.recovery_map()
    step = math.radians(1.0)
    for seed in range(10):
        truth, scan, guess = sc_.recovery_trial(seed)
        out = sm.match(m["field"], scan, guess[None], m["sc"], m["g"], 14, 14, 12, step)
        ex, ey, eth = sc_.pose_error(out["robot_in_world"][0], truth)
        gx, gy, gth = sc_.pose_error(guess, truth)
        top = np.sort(out["scores"].reshape(-1))[-2:]
        print("trial %d: off %.3f %.3f m %.2f deg -> %.3f %.3f m %.2f deg; score %d of %d (guess %d), runner-up %d" %
              (seed, gx, gy, math.degrees(gth), ex, ey, math.degrees(eth), out["score"][0], 255 * out["num_scored_beams"][0],
               out["score_at_guess"][0], top[0]))
        assert ex <= 0.05 and ey <= 0.05 and eth <= step, seed
        assert out["score"][0] > out["score_at_guess"][0]
