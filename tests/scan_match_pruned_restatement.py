"""Independent numpy restatement of pruned correlative scan matching (DESIGN.md section 4 "Pruned scan matching"), on top of
tests/scan_match_restatement.py (``end_cells``, ``rotated_guesses``, ``match``).

The bound plane P_l holds per cell the maximum of the field over the block of side 2^l that starts there; a block of shifts is
bounded by the sum of P_l under the beams' end cells moved to the block's first shift.  The search bounds every block of the top
level, scores the best block and the guess exactly, and descends level by level through the blocks whose bound reaches that
floor.  Its result is the exhaustive one, ties included; the library must give the same bits, statistics included.  Nothing here
knows the library.
"""
import numpy as np

import scan_match_restatement as sm

F = np.float32
MAX_LEVELS = 6
DEFAULT_LIST_ENTRIES = 1 << 20


def bound_planes(field, levels):
    """[P_0 .. P_levels]: P_l is (rows + s - 1, cols + s - 1) uint8 with s = 2^l, P_l[y + s - 1, x + s - 1] = the maximum of the
    field over the cells [x, x + s) x [y, y + s) inside the grid (0 if none): a 2 x 2 maximum of P_(l-1) at offset s / 2"""
    assert 0 <= levels <= MAX_LEVELS
    planes = [np.asarray(field, np.uint8)]
    rows, cols = planes[0].shape
    for l in range(1, levels + 1):
        s, h = 1 << l, 1 << (l - 1)
        prev = planes[-1]
        out = np.zeros((rows + s - 1, cols + s - 1), np.uint8)
        for b in (0, h):
            for a in (0, h):
                # out[Y, X] = max over a, b in {0, h} of prev[Y - b, X - a]: the four blocks of side h that make up the block of side s
                part = out[b:b + prev.shape[0], a:a + prev.shape[1]]
                np.maximum(part, prev, out=part)
        planes.append(out)
    return planes


def live_cells(ranges_k, guess_k, sc, g, wx, wy, ht, theta_step):
    """per rotation jj = 0 .. 2 ht: the end cells (x1, y1) int64 of the beams that are scored and that some shift of the window
    brings inside the grid (the others add 0 to every candidate and to every bound)"""
    rows, cols = g["rows"], g["cols"]
    out = []
    for jj in range(2 * ht + 1):
        if sc["num_beams"] == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))
            continue
        ok, x1, y1 = sm.end_cells(ranges_k[None], guess_k[None], sc, g, jj - ht, theta_step, ht)
        x, y = x1[0][ok[0]].astype(np.int64), y1[0][ok[0]].astype(np.int64)
        reach = (x + wx >= 0) & (x - wx < cols) & (y + wy >= 0) & (y - wy < rows)
        out.append((x[reach], y[reach]))
    return out


def sums_under(plane, s, cells, jj, ix, iy, wx, wy):
    """per entry e: the sum over the beams of rotation jj[e] of P(x1 + ix[e] - wx, y1 + iy[e] - wy), P = plane of block side s"""
    out = np.zeros(len(jj), np.int64)
    H, W = plane.shape
    p = plane.astype(np.int64)
    for j in np.unique(jj):
        x, y = cells[j]
        sel = np.nonzero(jj == j)[0]
        for c0 in range(0, len(sel), 4096):
            e = sel[c0:c0 + 4096]
            X = x[None, :] + (ix[e] - wx + s - 1)[:, None]
            Y = y[None, :] + (iy[e] - wy + s - 1)[:, None]
            ok = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
            out[e] = np.where(ok, p[np.clip(Y, 0, max(H - 1, 0)), np.clip(X, 0, max(W - 1, 0))] if H * W else 0, 0).sum(axis=1)
    return out


def dense_bounds(plane, s, cells, wx, wy, nbx, nby):
    """(rotations, nby, nbx) int64: the bound of every block of a level, beam by beam (``sums_under`` over all blocks, faster)"""
    H, W = plane.shape
    p = plane.astype(np.int64)
    U = np.zeros((len(cells), nby, nbx), np.int64)
    for j, (xs, ys) in enumerate(cells):
        for x, y in zip(xs, ys):
            X0, Y0 = int(x) - wx + s - 1, int(y) - wy + s - 1  # block b looks at column X0 + b s: inside the plane for b0 <= b < b1
            b0, b1 = max(0, -(X0 // s)), min(nbx, -(-(W - X0) // s))
            a0, a1 = max(0, -(Y0 // s)), min(nby, -(-(H - Y0) // s))
            if b0 < b1 and a0 < a1:
                U[j, a0:a1, b0:b1] += p[Y0 + a0 * s:Y0 + (a1 - 1) * s + 1:s, X0 + b0 * s:X0 + (b1 - 1) * s + 1:s]
    return U


def key_of(score, is_guess, flat):
    return (int(score) << 32) | (0x80000000 if is_guess else 0) | (0x7fffffff - int(flat))


def search(field, planes, cells, wx, wy, ht, levels, max_list_entries=0, trace=None):
    """one scan: (flat index of the winner or None after a fall-back, its score, the score at the guess, the statistics).
    trace: a dict that receives per level the evaluated blocks, their bounds and who survived (for the property tests)."""
    nx, ny, nt = 2 * wx + 1, 2 * wy + 1, 2 * ht + 1
    limit = max_list_entries if max_list_entries > 0 else DEFAULT_LIST_ENTRIES
    L = levels
    nbx = [-(-nx // (1 << l)) for l in range(L + 1)]
    nby = [-(-ny // (1 << l)) for l in range(L + 1)]
    st = {"num_candidates": nx * ny * nt, "num_evaluated": [0] * (MAX_LEVELS + 1), "num_survivors": [0] * (MAX_LEVELS + 1),
          "floor_score": 0, "seed_block": 0, "fell_back": 0, "seed_candidates": 0}
    s = 1 << L
    # 1. the dense top level
    flat = np.arange(nt * nby[L] * nbx[L], dtype=np.int64)
    jj, by, bx = flat // (nby[L] * nbx[L]), (flat // nbx[L]) % nby[L], flat % nbx[L]
    U = dense_bounds(planes[L], s, cells, wx, wy, nbx[L], nby[L]).reshape(-1)
    st["num_evaluated"][L] = len(flat)
    seed = int(np.argmax(U))  # (the first of the maxima: the lowest flat block index)
    st["seed_block"] = seed
    # 2. the guess and the seed block, exactly
    sx = np.arange(bx[seed] * s, min(bx[seed] * s + s, nx), dtype=np.int64)
    sy = np.arange(by[seed] * s, min(by[seed] * s + s, ny), dtype=np.int64)
    cx, cy = np.tile(sx, len(sy)), np.repeat(sy, len(sx))
    cj = np.full(len(cx), jj[seed], np.int64)
    st["seed_candidates"] = len(cx)
    cx, cy, cj = np.append(cx, wx), np.append(cy, wy), np.append(cj, ht)
    exact = sums_under(planes[0], 1, cells, cj, cx, cy, wx, wy)
    at_guess = int(exact[-1])
    guess_flat = (ht * ny + wy) * nx + wx
    best = 0
    for sc_, f in zip(exact, (cj * ny + cy) * nx + cx):
        best = max(best, key_of(sc_, f == guess_flat, f))
    floor = int(exact.max())
    st["floor_score"] = floor
    strict = floor == at_guess
    # 3. .. 4. the descent
    for l in range(L, 0, -1):
        alive = U > floor if strict else U >= floor
        st["num_survivors"][l] = int(alive.sum())
        if trace is not None:
            trace[l] = {"jj": jj, "by": by, "bx": bx, "U": U, "alive": alive}
        pj, py, px = jj[alive], by[alive], bx[alive]
        h = 1 << (l - 1)
        kids = [(pj, 2 * py + b, 2 * px + a) for b in (0, 1) for a in (0, 1)]
        jj = np.concatenate([k[0] for k in kids])
        by = np.concatenate([k[1] for k in kids])
        bx = np.concatenate([k[2] for k in kids])
        inside = (by * h < ny) & (bx * h < nx)
        jj, by, bx = jj[inside], by[inside], bx[inside]
        if len(jj) > limit:
            st["fell_back"] = 1
            st["num_evaluated"][0] = st["num_candidates"]
            return None, None, at_guess, st
        st["num_evaluated"][l - 1] = len(jj)
        U = sums_under(planes[l - 1], h, cells, jj, bx * h, by * h, wx, wy)
    if trace is not None:
        trace[0] = {"jj": jj, "by": by, "bx": bx, "U": U}
    for sc_, f in zip(U, (jj * ny + by) * nx + bx):
        best = max(best, key_of(sc_, f == guess_flat, f))
    return 0x7fffffff - (best & 0x7fffffff), best >> 32, at_guess, st


def evaluations(st, levels):
    """score evaluations of one search: the top-level bounds, the seed block, the guess and everything below"""
    return sum(st["num_evaluated"][:levels + 1]) + st["seed_candidates"] + 1


def match(field, ranges, guesses, sc, g, wx, wy, ht, theta_step, levels, max_list_entries=0, planes=None):
    """the members of srrg2_gridmap_match_result as arrays over the K scans (as scan_match_restatement.match, without the volume),
    and "stats": one dict per scan"""
    nb = sc["num_beams"]
    G = np.asarray(guesses, F).reshape(-1, 3, 3)
    K = G.shape[0]
    r = np.asarray(ranges, F).reshape(K, nb)
    nx, ny = 2 * wx + 1, 2 * wy + 1
    planes = bound_planes(field, levels) if planes is None else planes
    out = {"robot_in_world": np.zeros((K, 3, 3), F), "stats": []}
    for name in ("dx", "dy", "jtheta", "score", "score_at_guess", "num_scored_beams"):
        out[name] = np.zeros(K, np.int32)
    if K * nb:
        out["num_scored_beams"][:] = sm.gr.classify(r, sc)[0].sum(axis=1)
    for k in range(K):
        cells = live_cells(r[k], G[k], sc, g, wx, wy, ht, theta_step)
        flat, score, at_guess, st = search(field, planes, cells, wx, wy, ht, levels, max_list_entries)
        if flat is None:  # fell back: the whole window, exhaustively
            e = sm.match(field, r[k:k + 1], G[k:k + 1], sc, g, wx, wy, ht, theta_step)
            for name in ("dx", "dy", "jtheta", "score", "score_at_guess"):
                out[name][k] = e[name][0]
            out["robot_in_world"][k] = e["robot_in_world"][0]
            assert e["score_at_guess"][0] == at_guess
        else:
            dxi, rest = flat % nx, flat // nx
            dyi, jj = rest % ny, rest // ny
            dx, dy, j = dxi - wx, dyi - wy, jj - ht
            P = sm.rotated_guesses(G[k:k + 1], j, theta_step, ht)[0]
            with np.errstate(over="ignore", invalid="ignore"):
                P[0, 2] = P[0, 2] + F(dx) * g["res"]
                P[1, 2] = P[1, 2] + F(dy) * g["res"]
            out["robot_in_world"][k] = P
            out["dx"][k], out["dy"][k], out["jtheta"][k] = dx, dy, j
            out["score"][k], out["score_at_guess"][k] = score, at_guess
        out["stats"].append(st)
    return out
