"""Scene clouds past the two size thresholds of the scene kernels' launch geometry, and what the device has to make of them.
numpy only: the builders and references here know nothing of the library (tests/test_scene_large_cases.py checks them on the
CPU, tests/test_gpu_scene_large.py runs the device on them).

CAP: `blocks_for()` (csrc/scene_device.h) launches the one-thread-per-point kernels with at most 2048 workgroups of 256 threads;
a scene of more than CAP points sends every thread round its grid-stride loop a second time.

T * T: `launch_exclusive_scan` (csrc/kernels_prep.hip) scans tiles of T = SCAN_TILE elements, then the tile sums in ONE workgroup
that takes T sums per trip and carries their total to the next trip; the carry is used only beyond T tiles = T * T elements.
"""
import numpy as np

import normals_restatement as nr
import voxel_restatement as vr

F32, F64, I64 = np.float32, np.float64, np.int64
SCAN_TILE = 2048  # kernels_prep.hip: SCAN_THREADS * SCAN_ITEMS, the elements one workgroup of the exclusive scan takes
T = SCAN_TILE
CAP = 2048 * 256  # scene_device.h blocks_for(): threads of the largest grid a one-thread-per-point kernel gets
N_CAP = CAP + 2 * T + 1  # past the cap by two scan tiles and one point: no multiple of any workgroup or tile size
SCAN_SIZES = (T * T, T * T + 1, 2 * T * T + T + 1)  # one full trip over the sums; a 2nd trip of one sum; a 3rd, two carries


def features(n, seed):
    """(descriptors (n, 32) uint8, intensity (n,) float32)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.random(n, dtype=F32)


def _se3(t, deg):
    rx, ry, rz = np.deg2rad(np.asarray(deg, F64))
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.ascontiguousarray(np.hstack([Rz @ Ry @ Rx, np.asarray(t, F64).reshape(3, 1)]), F32)


def _se2(x, y, th):
    return np.array([[np.cos(th), -np.sin(th), x], [np.sin(th), np.cos(th), y], [0, 0, 1]], F32)


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


# ---- A: the keep flags of a ball clip, set by geometry with a wide margin ------------------------------------------------
SCAN_RANGE = 12.0
SCAN_MARKED_TILES = {2046: 1, 2047: 1500, 2048: 1000, 2049: 517}  # tile -> kept points, around the edge of the sums' first trip


def scan_case(n, dim):
    """dict: points, normals (n, dim) float32; mask (n,) bool -- what a ball clip of `range_max` around `pose` has to keep;
    pose, pose_far (keeps nothing), range_max.  Every kept point lies within 0.5 range of the robot, every other finite one
    beyond 2 range: no rounding decides a flag.  Per scan tile: tile 0 all kept, tile 1 none, the full ones among
    SCAN_MARKED_TILES that many, the others a random share between 2 % and 60 %; point n - 1 kept, point n - 2 NaN."""
    rng = np.random.default_rng(7919 * dim + n % 1000003)
    tiles = -(-n // T)
    share = rng.uniform(0.02, 0.6, tiles).astype(F32)
    mask = rng.random(n, dtype=F32) < np.repeat(share, T)[:n]
    mask[:T] = True
    mask[T:2 * T] = False
    for tile, kept in SCAN_MARKED_TILES.items():
        if (tile + 1) * T <= n:
            m = np.zeros(T, bool)
            m[rng.choice(T, kept, replace=False)] = True
            mask[tile * T:(tile + 1) * T] = m
    mask[n - 1], mask[n - 2] = True, False
    R = SCAN_RANGE
    centre = np.array([3.0, -2.0, 0.5], F32)[:dim]
    a = F32(0.5 * R / np.sqrt(dim) * 0.999)  # a cube inside the ball of 0.5 R
    off = (rng.random((n, dim), dtype=F32) * (2 * a) - a).astype(F32)
    far = np.flatnonzero(~mask)
    sign = np.where(rng.random(len(far), dtype=F32) < 0.5, F32(-1), F32(1))
    off[far, 0] = sign * (F32(2.001 * R) + F32(R) * rng.random(len(far), dtype=F32))  # one coordinate beyond 2 R
    pts = (off + centre).astype(F32)
    pts[n - 2] = np.nan
    nrm = rng.standard_normal((n, dim), dtype=F32)
    if dim == 3:
        pose, pose_far = _se3(centre, (10.0, 5.0, -20.0)), _se3(centre + F32(1000.0), (10.0, 5.0, -20.0))
    else:
        pose, pose_far = _se2(centre[0], centre[1], 0.7), _se2(centre[0] + 1000.0, centre[1] + 1000.0, 0.7)
    return {"points": pts, "normals": nrm, "mask": mask, "pose": pose, "pose_far": pose_far, "range_max": R, "centre": centre}


# ---- B: the clippers past CAP, with every field -----------------------------------------------------------------------------
def clip_case(dim, n=N_CAP, seed=5):
    """dict: points (about 0.1 % of them with a NaN / inf coordinate), unit normals, descriptors, intensity.  dim 3: around a
    camera looking along +z; dim 2: around a scanner"""
    rng = np.random.default_rng(seed + dim)
    if dim == 3:
        pts = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-1.0, 10.0, n)], 1).astype(F32)
    else:
        pts = rng.uniform(-12, 12, (n, 2)).astype(F32)
    src = rng.integers(0, n, n // 16)
    pts[rng.integers(0, n, n // 16)] = pts[src]  # exact duplicates: ties of depth / range
    bad = rng.choice(n, max(1, n // 1000), replace=False)
    pts[bad, rng.integers(0, dim, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), len(bad))
    desc, inten = features(n, seed + 10 + dim)
    return {"points": pts, "normals": _unit(rng.normal(size=(n, dim))), "descriptors": desc, "intensity": inten, "bad": np.sort(bad)}


BALL_RANGE = {3: 3.0, 2: 8.0}


def ball_poses(dim):
    if dim == 3:
        return [_se3((0.5, -0.4, 4.0), (10.0, 5.0, -20.0)), _se3((-0.7, 0.6, 5.0), (-4.0, 12.0, 30.0))]
    return [_se2(3.0, -2.0, 0.7), _se2(-2.5, 1.5, -1.1)]


CAMERA_ROWS, CAMERA_COLS = 480, 640
CAMERA_K = np.array([[512.0, 0, 319.5], [0, 512.0, 239.5], [0, 0, 1.0]], F32)
# (robot_in_local_map, sensor_in_robot or None, occlusion_margin): occlusion on, then off, into one clipped scene
PROJECTIVE_RUNS = [(_se3((0.1, -0.05, 0.2), (3.0, -2.0, 5.0)), _se3((0.02, 0.01, -0.03), (1.0, 2.0, -1.5)), 0.05),
                   (_se3((-0.15, 0.1, -0.1), (-4.0, 1.0, -6.0)), None, -1.0)]
# (num_beams, angle_min, angle_increment, robot_in_local_map, sensor_in_robot or None, occlusion_margin): the per-beam minimum in
# LDS tables (a margin wide enough to keep more than a scan tile of points), then in global memory (more beams than the LDS holds), then no occlusion test at all
SCAN_CLIP_RANGES = (2.0, 10.0)  # (range_min, range_max)
SCAN_RUNS = [(360, -np.pi, 2 * np.pi / 360, _se2(0.3, -0.2, 0.4), _se2(0.1, 0.05, -0.2), 0.5),
             (100_000, np.pi, -2 * np.pi / 100_000, _se2(-0.4, 0.1, -0.6), None, 0.0),
             (1081, -2.35619, 4.71238 / 1080, _se2(0.2, 0.3, 1.0), None, -1.0)]


def scan_minimum_in_lds(n, num_beams):
    """what srrg2_scene_clip_scan (csrc/scene.hip) takes for the per-beam minimum of a clip with occlusion: LDS tables when they
    fit (SRRG2_SCLIP_LDS_BINS = 8192 beams) and at least 20 workgroups each get 4 points per beam, else global atomics"""
    return num_beams <= 8192 and n // (4 * num_beams) >= 20


# ---- C: voxelize ------------------------------------------------------------------------------------------------------------
def voxelize_vectorised(points, leaf_size, dim=None, origin=(0.0, 0.0, 0.0), mode=vr.CENTROID, min_points=1, normals=None,
                        descriptors=None, intensity=None):
    """voxel_restatement.voxelize without its loop over the cells: the same arguments, the same dict, every value through the
    same operations in the same order.  The cells by np.unique on packed int64 keys; the fixed-point sums exact, int64, by a
    stable sort on the cell and np.add.reduceat."""
    P = vr._rows(points, F32)
    dim = P.shape[1] if dim is None else dim
    P = P[:, :dim]
    n = len(P)
    N = None if normals is None else vr._rows(normals, F32)[:, :dim]
    leaf = F64(F32(leaf_size))
    org = np.asarray(tuple(origin) + (0.0,) * (3 - len(origin)), F32)[:dim].astype(F64)
    e = vr.exponents(leaf_size, n)[0]
    en = vr.exponents(1.0, n)[0]
    part, cell = vr.cells_of(P, leaf_size, org.astype(F32), dim)
    idx = np.flatnonzero(part)
    occupied = most = with_normal = 0
    out_p, out_n = np.zeros((0, dim), F32), np.zeros((0, dim), F32)
    g, counts = np.zeros(0, np.int32), np.zeros(0, np.int32)
    if idx.size:
        cf = cell[idx]  # whole numbers, float64
        if not (np.abs(cf) < 2.0 ** 62).all():
            raise ValueError("voxelize_vectorised: cell coordinates beyond int64")
        ci = cf.astype(I64)
        rel = ci - ci.min(0)
        width = [int(w) + 1 for w in rel.max(0)]
        if int(np.prod([w for w in width], dtype=object)) >= 1 << 63:
            raise ValueError("voxelize_vectorised: the extent does not pack into an int64 key")
        key = rel[:, 0].copy()
        for d in range(1, dim):
            key = key * I64(width[d]) + rel[:, d]
        _, first, inv, cnt = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        occupied, most = len(cnt), int(cnt.max())
        by_rep = np.argsort(first, kind="stable")  # idx ascends: a cell's first occurrence is its lowest scene index
        rank = np.empty(occupied, I64)
        rank[by_rep] = np.arange(occupied)
        rep, k = idx[first[by_rep]], cnt[by_rep]  # per cell, in the order of the representatives
        slot = rank[inv]  # per participating point: its cell in that order
        order = np.argsort(slot, kind="stable")  # members cell by cell, ascending scene index within a cell
        start = np.r_[0, np.cumsum(k)[:-1]]
        p = P[rep].copy()
        nv = None if N is None else N[rep].copy()
        if mode == vr.CENTROID:
            corner = org[None, :] + cell[rep] * leaf  # one multiply, one add
            q = np.rint((P[idx].astype(F64) - corner[slot]) * F64(2.0) ** e).astype(I64)
            S = np.add.reduceat(q[order], start, axis=0)
            mean = (corner + (S.astype(F64) * F64(2.0) ** -e) / k.astype(F64)[:, None]).astype(F32)
            p[k > 1] = mean[k > 1]
            if N is not None:
                M = N[idx]
                with np.errstate(invalid="ignore"):
                    ok = (np.abs(M) < F32(2.0)).all(1)  # (finite and below 2 in magnitude: NaN and inf compare false)
                t = np.rint(np.where(ok[:, None], M, F32(0.0)).astype(F64) * F64(2.0) ** en).astype(I64)
                v = np.add.reduceat(t[order], start, axis=0).astype(F64)
                any_ok = np.add.reduceat(ok[order].astype(I64), start) > 0
                ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) if dim == 3 else \
                    np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
                good = any_ok & (ln > 0.0)
                with np.errstate(all="ignore"):
                    nv = np.where(good[:, None], v / ln[:, None], np.nan).astype(F32)
        emit = k >= min_points
        out_p, g, counts = p[emit], rep[emit].astype(np.int32), k[emit].astype(np.int32)
        if nv is not None:
            out_n = nv[emit]
            with_normal = int((~np.isnan(out_n).any(1)).sum())
    m = len(g)
    res = {"num_points": n, "num_finite": int(part.sum()), "num_occupied": occupied, "num_voxels": m,
           "num_with_normal": with_normal, "max_points_per_voxel": most}
    return {"points": np.ascontiguousarray(out_p, F32).reshape(m, dim),
            "normals": None if N is None else np.ascontiguousarray(out_n, F32).reshape(m, dim),
            "descriptors": None if descriptors is None else np.ascontiguousarray(descriptors)[g],
            "intensity": None if intensity is None else np.ascontiguousarray(intensity, F32)[g],
            "global_indices": g, "counts": counts, "result": res}


VOXEL_LEAF = 0.25


def voxel_many_cells(dim, n=N_CAP, seed=3):
    """dict: points, normals, leaf, cells_of_point (the intended cell of every finite point), expected numbers of cells.  n points
    over ALMOST n cells of a lattice: n // 200 cells hold two points, n // 1000 hold three, 0.025 % of the points are not
    finite and every other point has a cell to itself -- with n = N_CAP more than CAP cells are occupied.  Scene order is random.
    A tenth of the normals is bad (NaN, inf, a component of 2 or more)."""
    rng = np.random.default_rng(seed + dim)
    twos, threes, bad = n // 200, n // 1000, n // 4000
    ncell = n - bad - twos - 2 * threes
    side = int(np.ceil(ncell ** (1.0 / dim))) + 1
    assert side ** dim >= ncell
    flat = rng.choice(side ** dim, ncell, replace=False)
    cells = np.stack(np.unravel_index(flat, (side,) * dim), 1).astype(I64) - side // 2  # (negative cells too)
    owner = np.concatenate([np.arange(ncell), np.arange(twos), np.arange(twos, twos + threes), np.arange(twos, twos + threes)])
    owner = owner[rng.permutation(len(owner))]
    c = cells[owner]
    pts = ((c + rng.uniform(0.1, 0.9, c.shape)) * VOXEL_LEAF).astype(F32)
    pts = np.concatenate([pts, np.zeros((bad, dim), F32)])
    c = np.concatenate([c, np.zeros((bad, dim), I64)])
    order = rng.permutation(n)
    pts, c = pts[order], c[order]
    is_bad = order >= n - bad
    pts[is_bad, rng.integers(0, dim, bad)] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), bad)
    nrm = _unit(rng.normal(size=(n, dim)))
    some = rng.choice(n, n // 10, replace=False)
    nrm[some, rng.integers(0, dim, len(some))] = rng.choice(np.array([np.nan, np.inf, 2.0, -7.5, 1e30], F32), len(some))
    return {"points": pts, "normals": nrm, "leaf": VOXEL_LEAF, "cells": c, "finite": ~is_bad, "num_cells": ncell,
            "num_twos": twos, "num_threes": threes}


def voxel_lattice(n=T * T + T + 1, seed=4):
    """(n, 3) float32: n distinct cell centres of a unit-leaf lattice around the origin, in random order: every coordinate is a
    whole number plus one half -- exactly representable, half a leaf from every face -- and every point owns its cell"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0))) + 1
    flat = rng.choice(side ** 3, n, replace=False)
    cells = np.stack(np.unravel_index(flat, (side,) * 3), 1).astype(I64) - side // 2
    return (cells.astype(F64) + 0.5).astype(F32), cells


# ---- D: normals -------------------------------------------------------------------------------------------------------------
def _oddities(n_iso, n_dup, dim, far):
    """points that get no normal: lone ones (too few neighbours) and groups of six identical ones (a zero covariance:
    degenerate; six is min_neighbours or more in both dims), on a lattice of spacing 1 that starts at `far` on every axis"""
    k = n_iso + n_dup
    side = int(np.ceil(k ** (1.0 / dim))) + 1
    spots = (far + np.stack(np.unravel_index(np.arange(k), (side,) * dim), 1)).astype(F32)
    return np.concatenate([spots[:n_iso], np.repeat(spots[n_iso:], 6, axis=0)])


NORMALS_MAX_CURVATURE = 0.2
NORMALS_VIEW = (0.3, -0.2, 5.0)


def normals_curve(n=N_CAP, seed=6):
    """dict: points (n, 2), radius.  A wavy curve, laid out in rows of 100 m, sampled every third of the radius (about 6
    neighbours inside it) with noise of 0.15 radius across it; 0.2 % lone points, 0.1 % in groups of six identical
    ones, 0.1 % not finite; scene order is random"""
    rng = np.random.default_rng(seed)
    radius = 0.02
    n_iso, n_dup, n_bad = n // 500, n // 6000, n // 1000
    m = n - n_iso - 6 * n_dup
    s = (np.arange(m) + rng.uniform(-0.3, 0.3, m)) * (radius / 3.0)
    row, x = np.floor(s / 100.0), np.mod(s, 100.0)
    y = row * 1.0 + 0.1 * np.sin(2 * np.pi * x / 2.5) + rng.normal(scale=0.15 * radius, size=m)
    pts = np.concatenate([np.stack([x, y], 1).astype(F32), _oddities(n_iso, n_dup, 2, -50.0)])
    assert len(pts) == n
    pts = pts[rng.permutation(n)]
    bad = rng.choice(n, n_bad, replace=False)
    pts[bad, rng.integers(0, 2, n_bad)] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), n_bad)
    return {"points": pts, "radius": radius}


def normals_behind_a_dead_head(head=CAP, m=40_000, seed=8):
    """dict: points (head + m, 3), radius.  `head` points that are not finite, then m points of the noisy surfaces of
    normals_restatement.surface (about 10 neighbours), lone points and groups of identical ones among them, in random order:
    with head = CAP every point that takes part has a scene index of CAP or more"""
    rng = np.random.default_rng(seed)
    kinds = ["plane", "sphere", "cylinder", "crossing"]
    n_iso, n_dup = m // 200, m // 2400
    per = (m - n_iso - 6 * n_dup) // len(kinds)
    radius = float(0.09 * (5000.0 / per) ** 0.5 * 0.6)
    parts = [nr.surface(k, per if j else m - n_iso - 6 * n_dup - per * (len(kinds) - 1), seed + j, radius, 3) for j, k in enumerate(kinds)]
    live = np.concatenate(parts + [_oddities(n_iso, n_dup, 3, -20.0)])
    assert len(live) == m
    dead = np.zeros((head, 3), F32)
    dead[np.arange(head), rng.integers(0, 3, head)] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), head)
    return {"points": np.concatenate([dead, live[rng.permutation(m)]]), "radius": radius, "head": head}
