"""The cases the pruned scan-matching tests share (CPU: tests/test_scan_match_pruned_restatement.py, GPU:
tests/test_gpu_scan_match_pruned.py).  numpy only: nothing here calls the library.  The recovery setting is that of
tests/scan_match_cases.py; the rest are the shapes at which the new kernels of csrc/scan_match.hip can go wrong.

The launch caps and chunk sizes of the new kernels (scan_match.hip: enum { ..., BOUNDS_BLOCKS = 2048, TOP_BLOCKS = 2048,
SEED_BLOCKS = 1024, EXPAND_BLOCKS = 512, LIST_BLOCKS = 256, FALLBACK_BLOCKS = 2048 }), every kernel with workgroups of 256 threads:

BOUNDS_CAP    k_bounds_build writes one byte of a plane per thread and strides over the rest: a plane of more bytes sends every
              thread round again.
TOP_CAP       k_prune_top works on one tile per workgroup -- 256 blocks of one rotation of one scan -- and strides over the tiles
              beyond; where the tiles of a rotation do not divide the cap a workgroup's second trip has another chunk, another
              rotation and another scan than its first, on the same LDS.
SEED_CAP      k_prune_seed: one tile per workgroup, ceil((4^L + 1) / 256) tiles per scan.
EXPAND_CAP    k_prune_expand_top takes 256 top blocks of one scan per workgroup and trip, turned by the scan's index.
LIST_CAP      k_prune_level and k_prune_exact take 256 entries of one scan's list per workgroup and trip, turned the same way; a
              list of more entries than the cap is walked in several trips.
FALLBACK_CAP  k_prune_fallback: one candidate per thread of a scan that fell back.
"""
import functools
import math

import numpy as np

import gridmap_cases as gc
import gridmap_restatement as gr
import scan_match_cases as smc
import scan_match_pruned_restatement as sp
import scan_match_restatement as sm

F = np.float32
BOUNDS_CAP = 2048 * 256
TOP_CAP = 2048
SEED_CAP = 1024
EXPAND_CAP = 512 * 256
LIST_CAP = 256 * 256
FALLBACK_CAP = 2048 * 256
MEMBERS = ("dx", "dy", "jtheta", "score", "score_at_guess", "num_scored_beams")
STATS = ("num_candidates", "num_evaluated", "num_survivors", "floor_score", "seed_block", "fell_back")


@functools.lru_cache(maxsize=None)
def recovery_planes(levels=6):
    planes = sp.bound_planes(smc.recovery_map()["field"], levels)
    for p in planes:
        p.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def recovery_batch(n=10):
    """the scans and guesses of recovery trials 0 .. n - 1 as one batch, and their true poses"""
    trials = [smc.recovery_trial(t) for t in range(n)]
    out = (np.stack([t[0] for t in trials]).astype(F), np.concatenate([t[1] for t in trials]).astype(F),
           np.stack([t[2] for t in trials]).astype(F))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def drawn(rows, cols, nb, K=3, seed=3, R=2, lut=None, boxes=True, noise=0.004):
    """a room (with the two boxes of the recovery setting, or bare) drawn into a rows x cols grid from K poses: the grid, the
    scanner, the room, the poses, their ranges, the planes and the field of radius R; lut: a tuple, None = the default table"""
    g = gr.grid(rows, cols, 0.05, (-1.0, 0.5))
    a0, inc = gc.fan(nb)
    sc = gr.scanner(a0, inc, nb, range_min=0.02, range_max=20.0)
    room = gc.room_of(g)
    poses = gc.trajectory(room, K, seed)
    if boxes:
        ranges = smc.box_scans(room, smc.boxes_of(room), poses, sc, sigma=noise, seed=seed + 1)
    else:
        ranges = gc.room_scans(room, poses, sc, sigma=noise, seed=seed + 1)
    h, w = gr.new_planes(g)
    gr.integrate(h, w, ranges, poses, sc, g)
    table = sm.default_lut(R) if lut is None else np.array(lut, np.uint8)
    field = sm.likelihood(h, w, 1, 50, R, table)
    for a in (poses, ranges, h, w, field, table):
        a.setflags(write=False)
    return {"g": g, "sc": sc, "room": room, "poses": poses, "ranges": ranges, "hits": h, "misses": w, "field": field, "R": R, "lut": table}


def centre_pose(g):
    """the guess of ``localize``: the centre of cell (cols // 2, rows // 2) at heading 0"""
    P = np.eye(3, dtype=F)
    P[0, 2] = float(g["ox"]) + (g["cols"] // 2 + 0.5) * float(g["res"])
    P[1, 2] = float(g["oy"]) + (g["rows"] // 2 + 0.5) * float(g["res"])
    return P


def localize_window(g, theta_step):
    return g["cols"] // 2, g["rows"] // 2, int(math.ceil(math.pi / theta_step))


# (wx, wy, ht): half windows 0, 1, 3, 4, 7, 8 mixed over the axes, with and without rotations; at levels 1 .. 4 a block is 2 .. 16
# wide, so that every window here is tiled exactly, tiled with a hanging last block, and covered by one block that hangs over it
BLOCK_EDGES = ((0, 0, 0), (1, 0, 1), (0, 1, 0), (3, 4, 1), (4, 3, 0), (7, 8, 1), (8, 7, 0), (1, 8, 0), (8, 1, 2), (3, 3, 0), (7, 7, 1))


def caps_case():
    """past every cap at once, with few beams: an 800 x 700 grid (level 1 has 801 x 701 bytes > BOUNDS_CAP), 3 scans of 64 beams
    and a window of 301 x 301 x 9 at level 1: 3 x 9 x ceil(151^2 / 256) = 2 430 tiles > TOP_CAP, 205 209 top blocks per scan >
    EXPAND_CAP, 815 409 candidates > FALLBACK_CAP.  Scan 1 keeps a single return and the field is a plateau (radius 16, a table
    of all 255) that its guess lies off, so that its candidates tie by the ten thousand and its level-0 list is longer than
    LIST_CAP.  With a list limit the same call sends scans past FALLBACK_CAP (the test's second half)."""
    d = drawn(700, 800, 64, K=3, seed=5, R=16, lut=(255,) * 257, boxes=False)
    truth = gc.trajectory(d["room"], 3, 41)
    scans = np.array(gc.room_scans(d["room"], truth, d["sc"], sigma=0.004, seed=42), F)
    scans[1, :32] = scans[1, 33:] = np.nan
    guesses = np.stack([p @ gc.pose(*off, 0.03) for p, off in zip(truth, ((1.1, -0.9), (-3.0, -2.0), (1.1, -0.9)))]).astype(F)
    return d, scans, guesses, (150, 150, 4), math.radians(1.0)


def caps_level_case():
    """k_prune_level past LIST_CAP: the plateau map of ``caps_case``, a scanner of ONE beam, one scan whose guess lies off the
    plateau and a window of 301 x 301 x 25 at level 2: the list of level 1 holds more than LIST_CAP blocks"""
    d = drawn(700, 800, 64, K=3, seed=5, R=16, lut=(255,) * 257, boxes=False)
    sc = gr.scanner(0.0, 0.1, 1, range_min=0.02, range_max=20.0)
    truth = gc.trajectory(d["room"], 3, 41)[1:2]
    scans = np.array(gc.room_scans(d["room"], truth, sc), F)
    guesses = np.stack([p @ gc.pose(-3.0, -2.0, 0.03) for p in truth]).astype(F)
    return d, sc, scans, guesses, (150, 150, 12), math.radians(1.0)
