"""Independent numpy restatement of correlative scan matching against the occupancy grid (DESIGN.md section 4 "Correlative scan
matching"), on top of tests/gridmap_restatement.py (``compose``, ``beams``, ``render``) and ``adaptor_restatement.sincos``.

The field is a dilation of the occupied cells by a table over the squared cell distance; a candidate (j, dy, dx) turns the guess
by j steps, traces the scan's returns to their end cells exactly as the grid does, shifts them by (dx, dy) whole cells and sums
the field under them in integers.  The library must give the same bits.  Nothing here knows the library.
"""
import numpy as np

import gridmap_restatement as gr
from adaptor_restatement import sincos

F = np.float32
MAX_RADIUS = 16


def default_lut(R):
    n = R * R + 1
    return ((255 * (n - np.arange(n, dtype=np.int64))) // n).astype(np.uint8)


def occupied(hits, misses, min_observations=1, occupied_percent=50):
    v = gr.render(hits, misses, min_observations).astype(np.int64)
    return (v >= occupied_percent) & (v <= 100)


def likelihood(hits, misses, min_observations, occupied_percent, R, lut):
    """(rows, cols) uint8: per cell the maximum of lut[dx^2 + dy^2] over the occupied cells c + (dx, dy), dx^2 + dy^2 <= R^2"""
    return dilate(occupied(hits, misses, min_observations, occupied_percent), R, lut)


def dilate(occ, R, lut):
    lut = np.asarray(lut, np.uint8)
    assert 0 <= R <= MAX_RADIUS and lut.size == R * R + 1
    rows, cols = occ.shape
    field = np.zeros((rows, cols), np.uint8)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d2 = dx * dx + dy * dy
            if d2 > R * R:
                continue
            # cell (y, x) sees the occupied cell (y + dy, x + dx)
            y0, y1, x0, x1 = max(0, -dy), min(rows, rows - dy), max(0, -dx), min(cols, cols - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            seen = occ[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            part = field[y0:y1, x0:x1]
            np.maximum(part, np.where(seen, lut[d2], 0).astype(np.uint8), out=part)
    return field


def rotated_guesses(guesses, j, theta_step, half_steps_theta):
    """Pj = dm::se2_compose(guess, Rj) for K guesses -> (K, 3, 3) float32"""
    s, c = sincos(np.array([0.0 if half_steps_theta == 0 else float(j) * float(theta_step)], np.float64))
    cf, sf = F(c[0]), F(s[0])
    R = np.array([[cf, -sf, 0], [sf, cf, 0], [0, 0, 1]], F)
    P = gr.compose(guesses, R)
    out = np.zeros((P.shape[0], 3, 3), F)
    out[:, :2, :] = P
    out[:, 2, 2] = 1
    return out


def end_cells(ranges, guesses, sc, g, j, theta_step, half_steps_theta):
    """per beam of the (K, num_beams) batch at rotation j: is scored (a return the grid would trace), x1, y1"""
    b = gr.beams(ranges, rotated_guesses(guesses, j, theta_step, half_steps_theta), sc, g)
    return b["ret"] & b["traced"], b["x1"], b["y1"]


def volume(field, ranges, guesses, sc, g, wx, wy, ht, theta_step):
    """(K, 2 ht + 1, 2 wy + 1, 2 wx + 1) int32 scores, and the number of returns per scan"""
    nb = sc["num_beams"]
    K = int(np.asarray(guesses, F).size // 9)
    rows, cols = field.shape
    vol = np.zeros((K, 2 * ht + 1, 2 * wy + 1, 2 * wx + 1), np.int64)
    r = np.asarray(ranges, F).reshape(K, nb)
    returns = gr.classify(r, sc)[0].sum(axis=1).astype(np.int32) if K * nb else np.zeros(K, np.int32)
    if K * nb == 0 or rows * cols == 0:
        return vol.astype(np.int32), returns
    f = field.astype(np.int64)
    for jj in range(2 * ht + 1):
        ok, x1, y1 = end_cells(r, guesses, sc, g, jj - ht, theta_step, ht)
        for k in range(K):
            for x, y in zip(x1[k][ok[k]], y1[k][ok[k]]):
                # shifts (dyi, dxi) of the window under which the beam's cell lies inside the grid
                a0, a1 = max(0, wy - y), min(2 * wy + 1, rows + wy - y)
                b0, b1 = max(0, wx - x), min(2 * wx + 1, cols + wx - x)
                if a0 < a1 and b0 < b1:
                    vol[k, jj, a0:a1, b0:b1] += f[y + a0 - wy:y + a1 - wy, x + b0 - wx:x + b1 - wx]
    assert vol.max(initial=0) <= 255 * nb
    return vol.astype(np.int32), returns


def best(vol_k, wx, wy, ht):
    """flat index of the winner of one scan's volume: the highest score; among equals the guess, else the lowest index"""
    flat = vol_k.reshape(-1)
    guess = (ht * (2 * wy + 1) + wy) * (2 * wx + 1) + wx
    top = flat.max()
    return guess if flat[guess] == top else int(np.argmax(flat))


def match(field, ranges, guesses, sc, g, wx, wy, ht, theta_step):
    """the members of srrg2_gridmap_match_result as arrays over the K scans, and the volume"""
    vol, returns = volume(field, ranges, guesses, sc, g, wx, wy, ht, theta_step)
    K = vol.shape[0]
    nx, ny = 2 * wx + 1, 2 * wy + 1
    out = {"robot_in_world": np.zeros((K, 3, 3), F), "scores": vol, "num_scored_beams": returns}
    for name in ("dx", "dy", "jtheta", "score", "score_at_guess"):
        out[name] = np.zeros(K, np.int32)
    G = np.asarray(guesses, F).reshape(K, 3, 3)
    for k in range(K):
        flat = best(vol[k], wx, wy, ht)
        dxi, rest = flat % nx, flat // nx
        dyi, jj = rest % ny, rest // ny
        dx, dy, j = dxi - wx, dyi - wy, jj - ht
        P = rotated_guesses(G[k:k + 1], j, theta_step, ht)[0]
        with np.errstate(over="ignore", invalid="ignore"):
            P[0, 2] = P[0, 2] + F(dx) * g["res"]
            P[1, 2] = P[1, 2] + F(dy) * g["res"]
        out["robot_in_world"][k] = P
        out["dx"][k], out["dy"][k], out["jtheta"][k] = dx, dy, j
        out["score"][k], out["score_at_guess"][k] = vol[k].reshape(-1)[flat], vol[k, ht, wy, wx]
    return out
