"""Scan-matcher and grid-map calls past the launch caps of csrc/scan_match.hip and at the ray lengths and coordinates where the
walk of csrc/gridmap.hip has never been held to its contract, and what the device has to make of them.  numpy only: nothing here
calls the library (tests/test_map_large_cases.py proves on the CPU that each case reaches the path it is here for,
tests/test_gpu_map_large.py runs the device on them).  The drawn map and the guesses are those of tests/test_gpu_scan_match.py
(`_map`, `_guesses`: numpy only as well), imported where they are used.

PREP_CAP: k_match_prep works on one (scan, rotation, beam) triple per thread and is launched with at most MAX_PREP_BLOCKS
workgroups of 256 threads; more triples send every thread round its grid-stride loop again ("trip" t covers the triples
t * PREP_CAP .. (t + 1) * PREP_CAP - 1), and the triple's index is split into scan / rotation / beam there.

SCORE_CAP: k_match_score works on one tile of shifts per workgroup -- LX shifts of dx by TY shifts of dy of one rotation of one
scan -- and is launched with at most MAX_SCORE_BLOCKS workgroups; workgroup b takes the tiles b, b + SCORE_CAP, ...  Where a
(scan, rotation) has more than one tile and the tile count per scan does not divide SCORE_CAP, the second trip hands a workgroup
another (tx, ty) than the first: its shared beam list, its live count and its reduction words are reused under another `wide`,
`high` and `holds`.

MAX_STEPS, CELL_GUARD: the grid's own limits (tests/gridmap_restatement.py has them): a ray of up to 32 000 cells, a cell
coordinate inside [-2^30, 2^30).
"""
import functools
import math

import numpy as np

import gridmap_cases as gc
import gridmap_restatement as gr
import scan_match_restatement as sm

F = np.float32
PI = math.pi
# scan_match.hip: enum { ..., MAX_SCORE_BLOCKS = 8192, MAX_PREP_BLOCKS = 8192, ... }
# const int blocks = (int) std::min<long long>((prep_total + 255) / 256, MAX_PREP_BLOCKS);
# hipLaunchKernelGGL(k_match_prep, dim3(blocks), dim3(256), 0, st, A, prep_total, h->match_cells.p, aux);
PREP_CAP = 8192 * 256
# const int blocks = (int) std::min<long long>(tiles, MAX_SCORE_BLOCKS);
# hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, A, ..., tiles, (int) tiles_x, (int) tiles_y, ...);
SCORE_CAP = 8192


def score_tiling(wx, wy, ht, K):
    """dict(LX, TY, tiles_x, tiles_y, tiles) of srrg2_gridmap_match_scans' launch: lanes along dx 16, 32 or 64, whichever pads
    the row of nx shifts least (the wider on a tie), TY = (256 / LX) * 4 rows of dy
        if (nx <= 16) launch(k_match_score<16, 4>, 16, 64);
        else if ((nx + 31) / 32 * 32 < (nx + 63) / 64 * 64) launch(k_match_score<32, 4>, 32, 32);
        else launch(k_match_score<64, 4>, 64, 16);
        tiles_x = (nx + LX - 1) / LX, tiles_y = (ny + TY - 1) / TY;  tiles = tiles_x * tiles_y * nt * K"""
    nx, ny, nt = 2 * wx + 1, 2 * wy + 1, 2 * ht + 1
    if nx <= 16:
        LX, TY = 16, 64
    elif (nx + 31) // 32 * 32 < (nx + 63) // 64 * 64:
        LX, TY = 32, 32
    else:
        LX, TY = 64, 16
    tx, ty = (nx + LX - 1) // LX, (ny + TY - 1) // TY
    return dict(LX=LX, TY=TY, tiles_x=tx, tiles_y=ty, nt=nt, tiles=tx * ty * nt * K)


def tile_of(t, tile):
    """(tx, ty, jj, scan) of a tile index: k_match_score's own decomposition, tx fastest"""
    rest, tx = divmod(tile, t["tiles_x"])
    rest, ty = divmod(rest, t["tiles_y"])
    scan, jj = divmod(rest, t["nt"])
    return tx, ty, jj, scan


def winner_tiles(t, want, wx, wy):
    """(tx, ty) per scan of the tile that holds the winning shift"""
    return (want["dx"] + wx) // t["LX"], (want["dy"] + wy) // t["TY"]


# name -> (beams of the drawn map and the scanner, scans, (wx, wy, ht), theta_step, seed, guess offset in m, guess turn in rad)
MATCHES = {
    # 33 x 61 x 1081 = 2 176 053 triples > PREP_CAP: the last scan's triples lie wholly in trip 2
    "prep_cap": (1081, 33, (0, 0, 30), 0.01, 41, 0.12, 0.25),
    # nx = 33: LX = 64, TY = 16, tiles_y = 3 (the last row of tiles has high = 1); 23 x 121 x 3 = 8 349 tiles > SCORE_CAP, and
    # 8 192 is no multiple of 3: in trip 2 a workgroup starts at another ty
    "tile_stride_y": (65, 23, (16, 16, 60), 0.005, 51, 0.5, 0.25),
    # nx = 81: LX = 32, TY = 32, tiles_x = 3, tiles_y = 2; 60 x 25 x 6 = 9 000 tiles: another tx on the strided trip as well
    "tile_stride_xy": (65, 60, (40, 20, 12), 0.005, 61, 0.9, 0.05),
}


@functools.lru_cache(maxsize=None)
def match_case(name):
    """dict(drawn: the tuple of test_gpu_scan_match._map, sc, scans, guesses, window, step, want: scan_match_restatement.match);
    computed once and shared, everything read-only"""
    import test_gpu_scan_match as tm

    nb, K, (wx, wy, ht), step, seed, offset, turn = MATCHES[name]
    drawn = tm._map(64, 64, nb)
    g, sc, room, poses, ranges, h, w, field = drawn
    truth = gc.trajectory(room, K, seed)
    scans = gc.room_scans(room, truth, sc, sigma=0.004, seed=seed + 1)
    if name == "prep_cap":
        scans = gc.mixed(scans, seed + 2)
    guesses = tm._guesses(truth, seed + 3, offset=offset, turn=turn)
    want = sm.match(field, scans, guesses, sc, g, wx, wy, ht, step)
    for a in (scans, guesses) + tuple(want.values()):
        a.setflags(write=False)
    return dict(drawn=drawn, sc=sc, g=g, scans=scans, guesses=guesses, window=(wx, wy, ht), step=step, want=want)


# ---- the grid: rays of tens of thousands of steps, cells that are not convertible ------------------------------------------------
LONG_GRID = dict(rows=7, cols=9, resolution=0.05, origin=(0.0, 0.0))
RANGE_MAX = 1599.0  # 31 980 cells of 0.05 m: inside the cap of 32 000
NB = 64  # a full circle in 64 beams: beam 32 looks along the sensor's x axis, beam 48 along its y axis, beam 40 between them


def circle_scanner(nb=NB):
    return gr.scanner(-PI, 2 * PI / nb, nb, range_min=0.02, range_max=RANGE_MAX, clear_beyond_max=True)


@functools.lru_cache(maxsize=None)
def long_rays():
    """dict(g, sc, poses (6, 3, 3), ranges (6, 64), planes h / w and counters `want` of gridmap_restatement.integrate).
    Scans 0 .. 3: every range +inf, cleared out to range_max -- from inside the grid; from 800 m to its left (beam 32 crosses it
    after 16 000 steps, x-major); from 1 500 m below (beam 48 crosses it after 30 000 steps, y-major); from 1 100 m away on the
    diagonal (beam 40 crosses it after 15 600 steps, |dx| and |dy| nearly equal).  Scans 4 and 5: gridmap_cases.mixed over short
    returns with everything beyond range_max taken out again and ONE beam set to +inf -- one lane of the wave walks 31 980
    steps beside 63 that are dead or done after a few; from inside the grid, and from 800 m to the left with the long beam
    crossing the grid."""
    g = gr.grid(LONG_GRID["rows"], LONG_GRID["cols"], LONG_GRID["resolution"], LONG_GRID["origin"])
    sc = circle_scanner()
    poses = np.stack([gc.pose(0.21, 0.16, 0.3), gc.pose(-800.0, 0.17, 0.0), gc.pose(0.22, -1500.0, 0.0),
                      gc.pose(-780.0, -780.0 - 0.04, 0.0001), gc.pose(0.13, 0.22, -1.1), gc.pose(-800.0, 0.12, 0.0)])
    ranges = np.full((6, NB), np.inf, F)
    short = gc.mixed(np.random.default_rng(71).uniform(0.03, 0.3, (2, NB)).astype(F), 72)
    short[short > RANGE_MAX] = np.nan
    short[0, 11] = np.inf
    short[1, 32] = np.inf
    ranges[4:] = short
    h, w = gr.new_planes(g)
    want = gr.integrate(h, w, ranges, poses, sc, g)
    for a in (poses, ranges, h, w):
        a.setflags(write=False)
    return dict(g=g, sc=sc, poses=poses, ranges=ranges, h=h, w=w, want=want)


# a coordinate x with x / 0.05 beyond 2^30 = 1 073 741 824 is not convertible: 6e7 m (1.2e9 cells) is not, 5.3e7 m (1.06e9) is;
# float32 is 4 m coarse there.  53 687 088 m is the last float32 whose cell is below 2^30: a beam that leaves it in +x ends in a
# cell that is not.
FAR, NEAR, EDGE = 6.0e7, 5.3e7, 53687088.0
GUARD_GROUPS = {"inside": (0, 7), "beyond": (1, 2, 3), "within": (4, 5), "edge": (6,)}


@functools.lru_cache(maxsize=None)
def guard(nb=NB, origin=(0.0, 0.0)):
    """dict(g, sc, poses (8, 3, 3), ranges (8, nb), h, w, want): ordinary ranges of 0.05 .. 3 m (inside the grid up to 0.4 m, `edge`: 5 .. 1 500 m) from
    poses inside the grid (scans 0 and 7), at +-6e7 m where a cell is not convertible (1: x, 2: x and y, 3: y alone), at 5.3e7 m
    where it is (4, 5) and on the last convertible float32 (6).  nb = 32: a wave holds two scans, a drawing one beside a guarded
    one.  origin (0, -1e9): no y of any pose is convertible."""
    g = gr.grid(LONG_GRID["rows"], LONG_GRID["cols"], LONG_GRID["resolution"], origin)
    sc = circle_scanner(nb)
    poses = np.stack([gc.pose(0.21, 0.16, 0.3), gc.pose(FAR, 0.1, 0.5), gc.pose(-FAR, -FAR, 2.0), gc.pose(0.2, FAR, -1.0),
                      gc.pose(NEAR, 0.1, 0.7), gc.pose(-NEAR, NEAR, -2.5), gc.pose(EDGE, 0.2, 0.0), gc.pose(0.33, 0.08, -2.0)])
    rng = np.random.default_rng(81 + nb)
    ranges = rng.uniform(0.05, 3.0, (8, nb)).astype(F)
    ranges[[0, 7]] = rng.uniform(0.03, 0.4, (2, nb)).astype(F)  # (the grid is 0.45 m x 0.35 m)
    ranges[6] = rng.uniform(5.0, 1500.0, nb).astype(F)
    ranges = gc.mixed(ranges, 82)
    h, w = gr.new_planes(g)
    want = gr.integrate(h, w, ranges, poses, sc, g)
    for a in (poses, ranges, h, w):
        a.setflags(write=False)
    return dict(g=g, sc=sc, poses=poses, ranges=ranges, h=h, w=w, want=want)
